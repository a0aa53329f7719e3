"""Every leaf of the Gemm, Gemv and Reduce launchers in the two pieces of context state the eager tests never change: a recording that is replayed
(ctx->recording: a hipGraph submitted many times) and a CU-masked context (ctx->compute_units, ctx->uneven_xcds).

The rows are those of tests/test_gpu_epilogue.py (LEAVES) and tests/test_gpu_operands.py (EXTRA_LEAVES, RM_LEAVES, GEMV_LEAVES, REDUCE_PATHS, the fused
Gemv + Reduce shapes), on the same integer operands: every output bit is the f64 product rounded once (tests/_util.py special_product), whatever the
split of K or the order of accumulation, so a leaf that moves to another split or replays stale workspace cannot hide inside a tolerance.

replay   one fresh context per row:
  1. the first call on it inside a recording: records cleanly, or -- the rows of SCRATCH, the region the leaf grows (derived from the launchers) --
     raises WorkspaceMustGrow (status 8), and the recording still finishes;
  2. eager once, then the same call recorded: the same launch log (RECORD_LEAF pins the divergences recording causes);
  3. replayed on exact, special (+-Inf, NaN) and exact operands again, written with wg_buf_write between submits, the output reset to its prefill before
     each: bit for bit (special: NaN as a class), nothing outside the output view touched;
  4. a split-K row and a padded row eagerly on the same context (they overwrite the shared workspace), then a workspace regrow while the command buffer
     lives and canary buffers allocated after it: the next replay gives the model's bits and leaves the canaries alone;
  5. column-major Gemm rows: gemm_ex at each (alpha, beta) of AB_EXACT recorded, replayed on two C0: alpha * truth + beta * C0 rounded once.
  Reduce (every REDUCE_PATHS entry, f32 and f16, the five ops) and the fused Gemv + Reduce (every shape and case) the same way: steps 1-3 (and 4 for one
  op), against the C oracle.
cu248, cu224, cu100, cu8   module-scoped masked contexts: 248 CUs with the missing ones from one XCD (uneven_xcds: the Gemm stream of every bench.py
  rank), 224 and 100 spread over the XCDs (the two-rank tests' ranks; 100 is not a multiple of 8), 8 (one CU per XCD: most products many rounds deep).
  Gemm and Gemv rows on exact operands, plus special ones on cu248 and cu100; REDUCE_PATHS with their special data and a 2^20-element fast vector (its
  partial count reaches the 4 x CUs cap on cu8); the fused Gemv + Reduce cases. Each call logs the leaf CTX_LEAF names for that context where the CU
  count moves it (each entry derived from the launcher code), the full chip's leaf elsewhere.
"""
import numpy as np
import pytest

import _util as U
from test_gpu_epilogue import F16, F32, LEAVES, SENTINEL, Row, _lib, _upload, _wg
from test_gpu_operands import (AB_EXACT, EXTRA_LEAVES, GEMV_LEAVES, GEMV_REDUCE_CASES, REDUCE_PATHS, RM_LEAVES, Stored, _check_f16_edges, _data,
                               _gemm_call, _gemv_call, _gemv_reduce_operands, _ints, _klass, _reduce_data)

pytestmark = pytest.mark.gpu

GEMM_ROWS = LEAVES + EXTRA_LEAVES + RM_LEAVES
MASKED = {"cu248": (248, True), "cu224": (224, False), "cu100": (100, False), "cu8": (8, False)}
SPECIAL_ON = ("cu248", "cu100")

# ---- the scratch a recorded call needs on a fresh context ------------------------------------------------------------------------------------------
# row -> the region its leaf creates or grows before it launches, as the WG_ERR_WORKSPACE message names it (runtime.hip grow_scratch; gemm_f16.hip
# launch_tiles for the tile queues; api.hip wg_gemv_reduce for y and the arrival counter). Rows not listed need none and must record on a fresh context.
_WS, _PAD, _STAGE = "workspace of", "padding workspace", "staging workspace"
SCRATCH = {
    # Gemm: split-K slabs and tail partials (wg_ctx_workspace), padded operand copies (gemm_f16.hip / gemm_f32.hip fewrow: the padding region), views
    # that are not vec4-aligned (api.hip gemm_staged), the f16 tile scheduler's queues (created on first use)
    **dict.fromkeys(("f16_skinny_split", "f16_t128_split", "f16_m16_splitk", "f16_m16_tail", "f32_mid_split", "f32_mid_split_forced", "f32_fewrow_skinnyT",
                     "f32_skinny_split", "f32_skinny_panels", "f32_big_splitk", "f32_big_tail"), _WS),
    "f16_pad_c": _PAD, "f16_pad_k": _PAD, "f32_fewrow": _PAD, "f16_staged": _STAGE, "f32_staged": _STAGE,
    "f16_m16_queues": "tile queues",
    # Gemv: the partials of a split + combine (gemv.hip gemv_launch), the split-K of a hand-off to the Gemm kernels, staged vectors (api.hip gemv_staged).
    # (gemv.small needs none: it writes the output directly)
    **{"gemv:" + n: _WS for n in ("n_t1_split", "n_t8_split", "f16_n_t4_split", "t_t1_split", "t_t2_split", "f16_tcols_split", "f32_9rhs_gemm", "f32_5rhs_gemm",
                                  "f32_tr_8rhs_gemm", "f16_8rhs_gemm")},
    "gemv:f32_stage_v": _STAGE, "gemv:f16_stage_v": _STAGE,
    # Reduce: the two-pass kernel's partials (reduce.hip launch_fast); reduce.long and reduce.rows4 need none (one workgroup per vector)
    "reduce:reduce.fast/": _WS,
    # Gemv + Reduce: y in the transpose workspace, fused or not (api.hip wg_gemv_reduce); the fused kernel also needs its arrival counter (see the test)
    **{"gemv_reduce:" + leaf: "transpose workspace" for leaf in ("gemv.small_reduce/rl=2", "gemv.small_reduce/rl=4", "gemv.small_reduce/rl=8", "gemv_reduce.two>gemv>")},
}

# ---- recording: the leaf a recorded call logs where it is not the eager one --------------------------------------------------------------------------
RECORD_LEAF = {
    "f16_m16_balance": "f16.m16/ns=1",  # gemm_f16.hip launch_tiles: the calibrated shares are off while recording (a replay would reuse this flag epoch)
}

# ---- masked contexts: (context, row[, variant]) -> the whole log of the call there, where the CU count moves the row off the full chip's leaf ----------
# (cus below is the context's CU count; "full" is 256)
_TAIL2 = " f16.m16tail/ns=2 f16.tail_reduce"
CTX_LEAF = {
    # --- f16 Gemm (gemm_f16.hip, gemm_f32_skinny.hip) ---
    # f16 skinny: the split with the fewest rounds x (K / c + 256) over c <= K / 256 with c x 32 row blocks <= 4 cus + 32: 8 fills 256 CUs in one round;
    # 248 and 224 take 7 (8 would need two rounds), 100 takes 3 (96 blocks, one round), 8 takes 1 (c <= 2, and two splits cost more rounds)
    ("cu248", "f16_skinny_split"): "f16.skinny/ns=7 splitk.reduce/ns=7", ("cu224", "f16_skinny_split"): "f16.skinny/ns=7 splitk.reduce/ns=7",
    ("cu100", "f16_skinny_split"): "f16.skinny/ns=3 splitk.reduce/ns=3", ("cu8", "f16_skinny_split"): "f16.skinny/ns=1",
    # 128 x 128 split-K: only while 2 x 16 tiles <= cus -- not on 8 CUs
    ("cu8", "f16_t128_split"): "f16.t128/ns=1",
    # 256 x 256 tiles, 4096^2: 256 tiles = 8 tiles over 248 CUs, 32 over 224: the leftover round is cut along K (tail split, r x 2 <= cus, >= 3 stages
    # per split: 2 splits of K = 512, 4 of K = 1024); 100 CUs leave 56 (> 50: no tail), 8 CUs none
    ("cu248", "f16_m16_static"): "f16.m16/ns=1" + _TAIL2, ("cu224", "f16_m16_static"): "f16.m16/ns=1" + _TAIL2,
    ("cu248", "f16_m16_queues"): "f16.m16q/ns=1" + _TAIL2, ("cu224", "f16_m16_queues"): "f16.m16q/ns=1" + _TAIL2,
    # the calibrated shares need all 256 CUs: elsewhere the tail split as above, the plain launch on 100, and the tile queues on 8 (256 tiles >= 16 rounds)
    ("cu248", "f16_m16_balance"): "f16.m16/ns=1 f16.m16tail/ns=4 f16.tail_reduce", ("cu224", "f16_m16_balance"): "f16.m16/ns=1 f16.m16tail/ns=4 f16.tail_reduce",
    ("cu100", "f16_m16_balance"): "f16.m16/ns=1", ("cu8", "f16_m16_balance"): "f16.m16q/ns=1",
    # wg_splitk_plan: cus / 16 tiles, then whole stages per split (15 and 14 -> 13 splits of 320 k; 6 of 704 k); 8 CUs: 32 > 8, no split
    ("cu248", "f16_m16_splitk"): "f16.m16/ns=13 splitk.reduce/ns=13", ("cu224", "f16_m16_splitk"): "f16.m16/ns=13 splitk.reduce/ns=13",
    ("cu100", "f16_m16_splitk"): "f16.m16/ns=6 splitk.reduce/ns=6", ("cu8", "f16_m16_splitk"): "f16.m16/ns=1",
    # 272 tiles: 72 left over on 100 CUs (> 50: no tail), none on 8, where 272 tiles >= 16 rounds take the tile queues
    ("cu100", "f16_m16_tail"): "f16.m16/ns=1", ("cu8", "f16_m16_tail"): "f16.m16q/ns=1",
    # padded 1032^2 x 512 / 1024^2 x 1088: 25 / 16 tiles are >= 8 CUs, so the 128 x 128 family is out; 45 pairs of 256 x 128 tiles beat the continuous
    # walk's model at K = 512, not at K = 1088, where the walk takes it (K <= 4096, more than one round)
    ("cu8", "f16_pad_c"): "f16.pad/c>f16.t256x128", ("cu8", "f16_pad_k"): "f16.pad>f16.cont",
    # --- f32 Gemm (gemm_f32.hip, gemm_f32_skinny.hip, gemm_f32_mid.hip) ---
    # 64 x 16384 x 512: the unsplit 64 x 64 tile needs 256 tiles <= 2 cus; else the few-row kernel (rows 16384: 128 blocks, c x 128 <= 4 cus + 128)
    ("cu100", "f32_mid_unsplit"): "f32.skinnyT/ns=2 splitk.reduceT/ns=2", ("cu8", "f32_mid_unsplit"): "f32.skinnyT/ns=1",
    # mid_split_plan: 4 x 64 tiles in one round of 256; on 248, 224 and 100 three splits are the cheapest; 64 tiles > 8 CUs: no mid tile, the few-row kernel
    ("cu248", "f32_mid_split"): "f32.mid64x64/ns=3 splitk.reduce/ns=3", ("cu224", "f32_mid_split"): "f32.mid64x64/ns=3 splitk.reduce/ns=3",
    ("cu100", "f32_mid_split"): "f32.mid64x64/ns=3 splitk.reduce/ns=3", ("cu8", "f32_mid_split"): "f32.skinnyT/ns=1",
    # the transposed product 8192 x 96 x 256: the mid family's model picks 64 x 64 (one round, 256), 96 x 64 (248, 224: 64 x 64 would be 384 tiles, two
    # rounds), 96 x 96 (100), and on 8 CUs (short K, 2 x 32 tiles >= cus) the better of 128 x 64 / 64 x 128
    **{(w, "f32_fewrow", tr): ("f32.fewrow>" if tr else "f32.fewrow>transpose ") + f"f32.mid{t}/ns=1 transpose"
       for w, t in (("cu248", "96x64"), ("cu224", "96x64"), ("cu100", "96x96"), ("cu8", "128x64")) for tr in (False, True)},
    # few rows: 4096 rows = 32 blocks, 4 splits in one round of 256; 3 on 100; 1 on 8 (c x 32 <= 64)
    ("cu100", "f32_fewrow_skinnyT"): "f32.skinnyT/ns=3 splitk.reduceT/ns=3", ("cu8", "f32_fewrow_skinnyT"): "f32.skinnyT/ns=1",
    # few columns: as the f16 skinny plan at (K / c + 128): 8 / 7 / 7 / 3 / 1
    ("cu248", "f32_skinny_split"): "f32.skinny/ns=7 splitk.reduce/ns=7", ("cu224", "f32_skinny_split"): "f32.skinny/ns=7 splitk.reduce/ns=7",
    ("cu100", "f32_skinny_split"): "f32.skinny/ns=3 splitk.reduce/ns=3", ("cu8", "f32_skinny_split"): "f32.skinny/ns=1",
    # 8 panels x 4 row blocks = 32 blocks: 4 splits in one round on 256 / 248 / 224, 3 on 100, 1 on 8
    ("cu100", "f32_skinny_panels"): "f32.skinny/p=8,ns=3 splitk.reduce/ns=3", ("cu8", "f32_skinny_panels"): "f32.skinny/p=8,ns=1",
    # 512 tiles of 256 x 128: more than 2 cus on 248 and 224, 16 (32) left over, cut in 2 along K (pairs of tiles per CU, the leftover alone)
    ("cu248", "f32_big"): "f32.big/ns=1 f32.bigtail/ns=2 f32.tail_reduce", ("cu224", "f32_big"): "f32.big/ns=1 f32.bigtail/ns=2 f32.tail_reduce",
    # 8 tiles x ns in one round: 16 on 256, 12 on 100 (13 would take two); 8 CUs: every split costs as many rounds as it saves
    ("cu100", "f32_big_splitk"): "f32.big/ns=12 splitk.reduce/ns=12", ("cu8", "f32_big_splitk"): "f32.big/ns=1",
    # 272 tiles: 48 left over on 224 (cus / r = 4 splits), 72 of 2 x 100 on 100 (4 splits cheapest), none of 16 on 8
    ("cu224", "f32_big_tail"): "f32.big/ns=1 f32.bigtail/ns=4 f32.tail_reduce", ("cu100", "f32_big_tail"): "f32.big/ns=1 f32.bigtail/ns=4 f32.tail_reduce",
    ("cu8", "f32_big_tail"): "f32.big/ns=1",
    # --- Gemv (gemv.hip plan_nsplit, uses_t_lds, gemv_t_lds_plan; gemv_few_rhs hand-offs to the Gemm kernels) ---
    # gemv.small needs a split (nsplit > 1); N with >= cus row blocks and k <= 1024 is never split: 16 and 8 row blocks on 8 CUs
    ("cu8", "gemv:small_rl8"): "gemv>f32.gemv gemv.n/t=1,ns=1", ("cu8", "gemv:small_rl4"): "gemv>f32.gemv gemv.n/t=2,ns=1",
    ("cu8", "gemv:f16_small_rl4"): "gemv>f16.gemv gemv.n/t=1,ns=1",
    # N, one row block: 4 workgroups per CU -> 4 cus / (blocks) splits, capped by k / 64 = 64 (2 matrices: 16)
    ("cu8", "gemv:n_t1_split"): "gemv>f32.gemv gemv.n/t=1,ns=32 gemv.combine/ns=32", ("cu8", "gemv:n_t8_split"): "gemv>f32.gemv gemv.n/t=8,ns=16 gemv.combine/ns=16",
    ("cu8", "gemv:f16_n_t4_split"): "gemv>f16.gemv gemv.n/t=4,ns=32 gemv.combine/ns=32",
    # two right-hand sides, from 8 outputs per CU on: the vectors in the LDS (512 and 256 outputs >= 64)
    ("cu8", "gemv:t_t2"): "gemv>gemv.tlds/nr=2,c=2,th=1024", ("cu8", "gemv:t_t2_split"): "gemv>gemv.tlds/nr=2,c=1,th=1024",
    # half-wave per column: 128 workgroups >= 2 per CU on 8: unsplit, and then K = 4096 takes 8 loads in flight
    ("cu8", "gemv:f16_tcols_split"): "gemv>f16.gemv gemv.tcols/e=8,u=8,v=1,ns=1",
    # the LDS kernel's workgroup shape: the cheapest column-trips per slot for the context's CUs (gemv_t_lds_plan)
    ("cu100", "gemv:tlds_nr2_c1_256"): "gemv>gemv.tlds/nr=2,c=1,th=512", ("cu8", "gemv:tlds_nr2_c1_256"): "gemv>gemv.tlds/nr=2,c=4,th=1024",
    ("cu100", "gemv:tlds_nr2_c1_512"): "gemv>gemv.tlds/nr=2,c=1,th=1024", ("cu8", "gemv:tlds_nr2_c1_512"): "gemv>gemv.tlds/nr=2,c=4,th=1024",
    ("cu100", "gemv:tlds_nr8_c1_1024"): "gemv>gemv.tlds/nr=8,c=2,th=1024", ("cu8", "gemv:tlds_nr8_c1_1024"): "gemv>gemv.tlds/nr=8,c=4,th=1024",
    ("cu100", "gemv:tlds_nr8_c2"): "gemv>gemv.tlds/nr=8,c=4,th=1024", ("cu8", "gemv:tlds_nr8_c2"): "gemv>gemv.tlds/nr=8,c=4,th=1024",
    ("cu100", "gemv:tlds_nr4_c4"): "gemv>gemv.tlds/nr=4,c=2,th=1024", ("cu8", "gemv:tlds_nr4_batch"): "gemv>gemv.tlds/nr=4,c=1,th=1024",
    # hand-offs: the f32 few-column plan (8192 rows: 64 blocks -> 4 / 3 / 3 / 3 / 1 splits; 4096 rows: 8 / 7 / 7 / 3), the f16 128 x 128 split (32 tiles x 2 <=
    # cus); on 8 CUs 4096 outputs >= 128 per CU put 8 right-hand sides of GemvTr on the LDS kernel instead
    ("cu248", "gemv:f32_5rhs_gemm"): "gemv>f32.skinny/ns=3 splitk.reduce/ns=3", ("cu224", "gemv:f32_5rhs_gemm"): "gemv>f32.skinny/ns=3 splitk.reduce/ns=3",
    ("cu100", "gemv:f32_5rhs_gemm"): "gemv>f32.skinny/ns=3 splitk.reduce/ns=3", ("cu8", "gemv:f32_5rhs_gemm"): "gemv>f32.skinny/ns=1",
    ("cu248", "gemv:f32_tr_8rhs_gemm"): "gemv>f32.skinny/ns=7 splitk.reduce/ns=7", ("cu224", "gemv:f32_tr_8rhs_gemm"): "gemv>f32.skinny/ns=7 splitk.reduce/ns=7",
    ("cu100", "gemv:f32_tr_8rhs_gemm"): "gemv>f32.skinny/ns=3 splitk.reduce/ns=3", ("cu8", "gemv:f32_tr_8rhs_gemm"): "gemv>gemv.tlds/nr=8,c=4,th=1024",
    ("cu8", "gemv:f16_8rhs_gemm"): "gemv>f16.t128/ns=1",
    # --- Reduce: the two-pass kernel's partials, min(n / 16 Ki, 4 cus) ---
    ("cu8", "reduce:fast-1048576"): "reduce.fast/np=32",
    # --- Gemv + Reduce: fused only where wg_gemv would take gemv.small (see above); the two-launch form's Gemv splits 4 cus / 32 blocks ways (<= 16) ---
    ("cu8", "gemv_reduce:2048x512"): "gemv_reduce.two>gemv>f32.gemv gemv.n/t=1,ns=1 reduce.rows4/al=1",
    ("cu8", "gemv_reduce:4096x1024"): "gemv_reduce.two>gemv>f32.gemv gemv.n/t=1,ns=1 reduce.rows4/al=1",
    ("cu100", "gemv_reduce:8192x1024"): "gemv_reduce.two>gemv>f32.gemv gemv.n/t=1,ns=13 gemv.combine/ns=13 reduce.rows4/al=1",
    ("cu8", "gemv_reduce:8192x1024"): "gemv_reduce.two>gemv>f32.gemv gemv.n/t=1,ns=1 reduce.rows4/al=1",
}


def _assert_leaf(log, where, key, default, tr=None, not_=None, what=""):
    """The call on a masked context logged CTX_LEAF's whole log for it, or -- no entry -- the full chip's tag(s)."""
    moved = CTX_LEAF.get((where, key, tr), CTX_LEAF.get((where, key)))
    if moved is not None:
        assert log == moved, f"{what} on {where}: expected {moved!r} (the CU count moves it), took {log!r}"
    else:
        assert Row.took(default, log, not_), f"{what} on {where}: expected the full chip's {default!r}, took {log!r}"


class _Knobs:
    """A row's knobs on one context (wg_ctx_set_tuning), restored on exit."""

    def __init__(self, inst, knobs):
        self.inst, self.knobs, self.saved = inst, knobs, {}

    def __enter__(self):
        for k, v in self.knobs.items():
            self.saved[k] = self.inst.set_tuning(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.inst.set_tuning(k, v)


@pytest.fixture(scope="module")
def masked():
    """The masked contexts, created on first use and closed at module teardown."""
    wg, made = _wg(), {}

    def get(where):
        if where not in made:
            n, one_xcd = MASKED[where]
            made[where] = wg.GpuInstance.new(0, cu_count=n, one_xcd=one_xcd)
        return made[where]

    yield get
    for inst in made.values():
        inst.sync()
        inst.close()


@pytest.fixture
def fresh():
    """A context of its own (empty scratch, no tile queues, no arrival counter); closed after the test."""
    inst = _wg().GpuInstance.new(0)
    yield inst
    inst.sync()
    inst.close()


class Recording:
    """A recording on `inst`'s context (wg_encoder_begin .. wg_encoder_finish): `call` runs inside it; `cb` is the command buffer, destroyed by `destroy`."""

    def __init__(self, inst):
        self.inst = inst
        self.enc = inst.device().create_command_encoder(record=True)
        self.cb = None

    def finish(self):
        self.cb = self.enc.finish()
        return self

    def submit(self):
        self.inst.queue().submit([self.cb])

    def destroy(self):
        if self.cb is not None and self.cb._h:
            _lib().lib.wg_cmdbuf_destroy(self.cb._h)
            self.cb._h = None


def _record(inst, call):
    """(the recording, its log) of `call` recorded on `inst`."""
    rec = Recording(inst)
    try:
        call()
    finally:
        rec.finish()
    return rec, inst.take_path()


def _first_call_recorded(inst, call, region, what):
    """Step 1: the first call on a fresh context inside a recording."""
    wg = _wg()
    inst.take_path()
    rec = Recording(inst)
    raised = None
    try:
        call()
    except wg.WorkspaceMustGrow as e:
        raised = e
    rec.finish()  # (the recording is still well-formed)
    log = inst.take_path()
    rec.destroy()
    if region is None:
        assert raised is None, f"{what}: needs no scratch, but recording on a fresh context raised {raised}"
    else:
        assert raised is not None, f"{what}: grows the {region} first, yet recorded on a fresh context without it [{log}]"
        assert raised.status == 8 and region in str(raised) and "recording" in str(raised), (what, region, raised.status, str(raised))


def _flat(st, X):
    """The parent buffer of Stored `st` with X in its view (what Stored uploads at creation)."""
    S = np.transpose(X, (1, 0, 2)) if st.tr else X
    flat = st.base.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        flat[st.idx] = S.astype(st.base.dtype)
    return flat


def _write(inst, st, X):
    inst.queue().write_buffer(st.buf, 0, _flat(st, X))


def _canaries(inst):
    """Buffers allocated after a regrow: a replay that still writes into the freed region lands in one of them."""
    return [_upload(inst, np.full((1 << 20) * k // 4, 7.0, np.float32)) for k in (1, 1, 2, 2, 4, 4, 8)]


def _check_canaries(inst, canaries, what):
    for c in canaries:
        assert (c.read(inst.device()) == 7.0).all(), f"{what}: a replay wrote into memory allocated after the regrow"


# intruders for step 4: eager calls that take the shared workspace (split-K) and the padding workspace, sized past what most rows recorded
_INTRUDERS = [r for r in LEAVES if r.name in ("f16_t128_split", "f16_pad_c")]


def _intrude(inst):
    """Step 4: a split-K row and a padded row eagerly on `inst`, then the workspace grown past both, then canaries."""
    rng = np.random.default_rng(4)
    for r in _INTRUDERS:
        with _Knobs(inst, r.knobs):
            a = Stored(inst, _ints(rng, (r.M, r.K, r.mats)), r.dtype, "dense")
            b = Stored(inst, _ints(rng, (r.K, r.N, r.mats)), r.dtype, "dense")
            out = Stored(inst, np.zeros((r.M, r.N, r.mats)), r.dtype, "dense", fill=SENTINEL[r.dtype])
            inst.take_path()
            _gemm_call(inst, r, False, out, a, b)
            log = inst.take_path()
            assert Row.took(r.leaf, log), f"intruder {r.name}: took {log!r}"
    inst.sync()
    inst.device().reserve_workspace(96 << 20)  # (past anything a row here records: the region its graph holds is retired, not freed)
    return _canaries(inst)


def _dirty_workspace(inst):
    """Fills the start of `inst`'s workspace with f32 split-K partials (integer sums, mostly nonzero): a forced four-way split of the mid 64 x 64 tile."""
    r = next(r for r in LEAVES if r.name == "f32_mid_split_forced")
    rng = np.random.default_rng(8)
    with _Knobs(inst, r.knobs):
        a = Stored(inst, _ints(rng, (r.M, r.K, 1)), F32, "dense")
        b = Stored(inst, _ints(rng, (r.K, r.N, 1)), F32, "dense")
        out = Stored(inst, np.zeros((r.M, r.N, 1)), F32, "dense")
        inst.take_path()
        _gemm_call(inst, r, False, out, a, b)
        assert inst.take_path() == r.leaf


# --------------------------------------------------------------------------------------------------------
# Gemm
# --------------------------------------------------------------------------------------------------------
WHERE = ("replay",) + tuple(MASKED)
GEMM_PARAMS = [pytest.param(r, tr, w, id=f"{r.name}-{'tr' if tr else 'nn'}-{w}") for r in GEMM_ROWS for tr in r.variants for w in WHERE]


def _gemm_setup(inst, row, tr, A, B):
    rm = getattr(row, "api", "cm") == "rm"
    a = Stored(inst, A, row.dtype, "dense", tr=tr and not rm)
    b = Stored(inst, B, row.dtype, "dense", tr=rm)
    out = Stored(inst, np.full((A.shape[0], B.shape[1], A.shape[2]), np.nan), row.dtype, "dense", tr=rm, fill=SENTINEL[row.dtype])
    return a, b, out


@pytest.mark.parametrize("row,tr,where", GEMM_PARAMS)
def test_gemm_leaf_in_context(request, masked, row, tr, where):
    d = _data((row.name, tr), row.M * 7 + row.K * 5 + row.N * 3 + row.mats + int(tr), row.dtype, row.M, row.K, row.N, row.mats)
    if row.dtype == F16:
        _check_f16_edges(d["truth"])
    if where == "replay":
        _gemm_replay(request.getfixturevalue("fresh"), row, tr, d)
    else:
        _gemm_masked(masked(where), where, row, tr, d)


def _gemm_masked(inst, where, row, tr, d):
    with _Knobs(inst, row.knobs):
        for case in ("exact", "special") if where in SPECIAL_ON else ("exact",):
            A, B, want = (d["A"], d["B"], d["want"]) if case == "exact" else (d["As"], d["Bs"], d["want_s"])
            a, b, out = _gemm_setup(inst, row, tr, A, B)
            inst.take_path()
            _gemm_call(inst, row, tr, out, a, b)
            log = inst.take_path()
            _assert_leaf(log, where, row.name, row.leaf, tr, what=f"{row.name} ({case})")
            got = out.read(f"{row.name} on {where} ({case})")
            if case == "exact":
                U.assert_bits_equal(got, want, f"{row.name} on {where} [{log}]")
            else:
                U.assert_same_class_bits(got, want, f"{row.name} special on {where} [{log}]")


def _gemm_replay(inst, row, tr, d):
    dtype, (M, N, Z) = row.dtype, (row.M, row.N, row.mats)
    name = f"{row.name}-{'tr' if tr else 'nn'}"
    with _Knobs(inst, row.knobs):
        a, b, out = _gemm_setup(inst, row, tr, d["A"], d["B"])
        prefill = np.full((M, N, Z), np.nan)
        call = lambda: _gemm_call(inst, row, tr, out, a, b)
        # 1. the first call of the context, recorded
        _first_call_recorded(inst, call, SCRATCH.get(row.name), name)
        # 2. eager once, then recorded: the same launches
        call()
        eager = inst.take_path()
        assert Row.took(row.leaf, eager), f"{name} eager: expected {row.leaf!r}, took {eager!r}"
        U.assert_bits_equal(out.read("eager"), d["want"], f"{name} eager [{eager}]")
        rec, log = _record(inst, call)
        try:
            want_log = RECORD_LEAF.get(row.name)
            if want_log is None:
                assert log == eager, f"{name}: recorded {log!r}, eager {eager!r}"
            else:
                assert Row.took(want_log, log) and log != eager, f"{name}: recorded {log!r}, expected {want_log!r}"
            # 3. replays on new data: exact -> special -> exact
            for case in ("exact", "special", "exact"):
                A, B, want = (d["A"], d["B"], d["want"]) if case == "exact" else (d["As"], d["Bs"], d["want_s"])
                _write(inst, a, A)
                _write(inst, b, B)
                _write(inst, out, prefill)
                rec.submit()
                got = out.read(f"{name} replay {case}")
                if case == "exact":
                    U.assert_bits_equal(got, want, f"{name} replay {case} [{log}]")
                else:
                    U.assert_same_class_bits(got, want, f"{name} replay {case} [{log}]")
            # 4. other rows' eager calls and a regrow while the command buffer lives
            canaries = _intrude(inst)
            _write(inst, out, prefill)
            rec.submit()
            U.assert_bits_equal(out.read(f"{name} replay after the regrow"), d["want"], f"{name} replay after other rows and a regrow [{log}]")
            _check_canaries(inst, canaries, name)
        finally:
            rec.destroy()
        # 5. gemm_ex recorded (column-major rows)
        if getattr(row, "api", "cm") == "rm":
            return
        rng = np.random.default_rng(M + N)
        c0s = (_ints(rng, (M, N, Z)), _ints(rng, (M, N, Z)))
        _write(inst, a, d["A"])
        _write(inst, b, d["B"])
        for alpha, beta in AB_EXACT:
            _write(inst, out, c0s[0])
            _gemm_call(inst, row, tr, out, a, b, alpha, beta)
            eager = inst.take_path()
            assert Row.took(row.leaf, eager) or Row.took(row.ab, eager, row.not_ab), f"{name} ({alpha}, {beta}): took {eager!r}"
            rec, log = _record(inst, lambda: _gemm_call(inst, row, tr, out, a, b, alpha, beta))
            try:
                assert log == eager or (row.name in RECORD_LEAF and Row.took(RECORD_LEAF[row.name], log)), f"{name} ({alpha}, {beta}): recorded {log!r}, eager {eager!r}"
                for c0 in c0s:
                    _write(inst, out, c0)
                    rec.submit()
                    with np.errstate(over="ignore"):
                        want = (alpha * d["truth"] + beta * c0 + 0.0).astype(dtype)
                    U.assert_bits_equal(out.read(f"{name} gemm_ex({alpha}, {beta}) replay"), want, f"{name} gemm_ex({alpha}, {beta}) replay [{log}]")
            finally:
                rec.destroy()


# --------------------------------------------------------------------------------------------------------
# Gemv
# --------------------------------------------------------------------------------------------------------
GEMV_PARAMS = [pytest.param(r, w, id=f"{r.name}-{w}") for r in GEMV_LEAVES for w in WHERE]


def _gemv_setup(inst, row, A, V):
    m = Stored(inst, A, row.dtype, "dense", tr=row.tr, ld_mult=row.ld_mult)  # (GemvTr: m = op(m)^T)
    vl = "odd" if row.vodd else "dense"
    v = Stored(inst, V, row.dtype, vl)
    out = Stored(inst, np.full((A.shape[0], V.shape[1], A.shape[2]), np.nan), row.dtype, vl, fill=SENTINEL[row.dtype])
    return m, v, out


def _gemv_data(row):
    ro, k = (row.C, row.R) if row.tr else (row.R, row.C)
    return _data(("gemv", row.name), ro * 7 + k * 5 + row.nrhs * 3 + row.mats + int(row.tr), row.dtype, ro, k, row.nrhs, row.mats)


@pytest.mark.parametrize("row,where", GEMV_PARAMS)
def test_gemv_leaf_in_context(request, masked, row, where):
    d = _gemv_data(row)
    if row.dtype == F16:
        _check_f16_edges(d["truth"])
    if where == "replay":
        _gemv_replay(request.getfixturevalue("fresh"), row, d)
        return
    inst = masked(where)
    with _Knobs(inst, row.knobs):
        for case in ("exact", "special") if where in SPECIAL_ON else ("exact",):
            A, V, want = (d["A"], d["B"], d["want"]) if case == "exact" else (d["As"], d["Bs"], d["want_s"])
            m, v, out = _gemv_setup(inst, row, A, V)
            inst.take_path()
            _gemv_call(inst, row, out, m, v)
            log = inst.take_path()
            _assert_leaf(log, where, "gemv:" + row.name, row.leaf, not_=row.not_, what=f"{row.name} ({case})")
            got = out.read(f"{row.name} on {where} ({case})")
            if case == "exact":
                U.assert_bits_equal(got, want, f"{row.name} on {where} [{log}]")
            else:
                U.assert_same_class_bits(got, want, f"{row.name} special on {where} [{log}]")


def _gemv_replay(inst, row, d):
    with _Knobs(inst, row.knobs):
        m, v, out = _gemv_setup(inst, row, d["A"], d["B"])
        prefill = np.full(d["want"].shape, np.nan)
        call = lambda: _gemv_call(inst, row, out, m, v)
        _first_call_recorded(inst, call, SCRATCH.get("gemv:" + row.name), row.name)
        call()
        eager = inst.take_path()
        assert Row.took(row.leaf, eager, row.not_), f"{row.name} eager: expected {row.leaf!r}, took {eager!r}"
        U.assert_bits_equal(out.read("eager"), d["want"], f"{row.name} eager [{eager}]")
        rec, log = _record(inst, call)
        try:
            assert log == eager, f"{row.name}: recorded {log!r}, eager {eager!r}"
            for case in ("exact", "special", "exact"):
                A, V, want = (d["A"], d["B"], d["want"]) if case == "exact" else (d["As"], d["Bs"], d["want_s"])
                _write(inst, m, A)
                _write(inst, v, V)
                _write(inst, out, prefill)
                rec.submit()
                got = out.read(f"{row.name} replay {case}")
                if case == "exact":
                    U.assert_bits_equal(got, want, f"{row.name} replay {case} [{log}]")
                else:
                    U.assert_same_class_bits(got, want, f"{row.name} replay {case} [{log}]")
            canaries = _intrude(inst)
            _write(inst, out, prefill)
            rec.submit()
            U.assert_bits_equal(out.read(f"{row.name} replay after the regrow"), d["want"], f"{row.name} replay after other rows and a regrow [{log}]")
            _check_canaries(inst, canaries, row.name)
        finally:
            rec.destroy()


# --------------------------------------------------------------------------------------------------------
# Reduce
# --------------------------------------------------------------------------------------------------------
FAST_LONG = ("fast", 1 << 20, 0, "reduce.fast/np=64")  # 64 partials of 16 Ki elements (reduce.hip launch_fast) -- 4 x CUs caps them at 32 on cu8
REDUCE_WHERE = ("replay",) + tuple(MASKED)
REDUCE_PARAMS = ([pytest.param(path, n, off, leaf, dt, w, id=f"{path}-{n}-{off}-{np.dtype(dt).name}-{w}")
                  for path, n, off, leaf in REDUCE_PATHS for dt in (F32, F16) for w in REDUCE_WHERE] +
                 [pytest.param(*FAST_LONG, dt, w, id=f"fast-long-{np.dtype(dt).name}-{w}") for dt in (F32, F16) for w in tuple(MASKED)])
REDUCE_OPS = (("Min", "minmax"), ("Max", "minmax"), ("Sum", "sum"), ("SqNorm", "sum"), ("Prod", "prod"))


class _ReduceCase:
    """One REDUCE_PATHS entry on one context: its input buffer (NaN before and after the view) and result, the call, and the oracle's bits."""

    def __init__(self, inst, path, n, off, dtype):
        wg = _wg()
        self.inst, self.path, self.n, self.off, self.dtype = inst, path, n, off, dtype
        self.cols = 3 if path == "batched" else 1
        self.t = _upload(inst, np.full(off + n * self.cols + 5, np.nan, dtype))
        self.res = _upload(inst, np.full(self.cols, np.nan, dtype))
        self.view = wg.GpuTensorView(wg.ViewShape((n, self.cols, 1), n, n * self.cols, off), self.t, 2 if self.cols > 1 else 1)

    def xs(self, x):
        return np.concatenate([np.roll(x, 7 * c) for c in range(self.cols)]).astype(self.dtype)  # (as test_reduce_special_values)

    def write(self, xs):
        self.inst.queue().write_buffer(self.t, 0, np.concatenate([np.full(self.off, np.nan, self.dtype), xs, np.full(5, np.nan, self.dtype)]))
        self.inst.queue().write_buffer(self.res, 0, np.full(self.cols, np.nan, self.dtype))

    def call(self, op):
        wg, dev = _wg(), self.inst.device()
        red, shapes = wg.Reduce.new(dev, wg.ReduceOp[op]), wg.ViewShapeBuffers()
        f = {"batched": red.dispatch_batched, "fast": red.dispatch_fast}.get(self.path, red.dispatch)
        enc = dev.create_command_encoder()
        with enc.compute_pass("reduce", None) as p:
            f(dev, shapes, p, self.view, self.res)

    def want(self, oracle_c, op, xs):
        from oracle import wgsl_oracle as wo
        x32, n = xs.astype(np.float32), self.n
        with np.errstate(over="ignore", invalid="ignore"):
            return np.array([oracle_c.reduce(int(getattr(wo, op.upper())), x32, wo.Shape(n, 1, 1, n, n, c * n)) for c in range(self.cols)],
                            np.float32).astype(self.dtype)

    def leaf(self, op, default):
        # (Min / Max of one long vector: the two-pass kernels -- wgk_reduce)
        return "reduce.fast/" if self.path == "single" and self.n >= 65536 and op in ("Min", "Max") else default


def _reduce_cases(n, off, dtype, fam):
    return _reduce_data(np.random.default_rng(n + off + (dtype == F16)), n, fam, dtype)


@pytest.mark.parametrize("path,n,off,leaf,dtype,where", REDUCE_PARAMS)
def test_reduce_in_context(request, masked, oracle_c, path, n, off, leaf, dtype, where):
    inst = request.getfixturevalue("fresh") if where == "replay" else masked(where)
    rc = _ReduceCase(inst, path, n, off, dtype)
    if where != "replay":
        if n == FAST_LONG[1]:  # (stale values past the partials this context's pass 1 writes: a pass 2 that folded more of them would show)
            _dirty_workspace(inst)
        for op, fam in REDUCE_OPS:
            for case, x in _reduce_cases(n, off, dtype, fam):
                xs = rc.xs(x)
                rc.write(xs)
                inst.take_path()
                rc.call(op)
                got = rc.res.read(inst.device())
                log = inst.take_path()
                _assert_leaf(log, where, f"reduce:{path}-{n}", rc.leaf(op, leaf), what=f"{path} n={n} {op}")
                want = rc.want(oracle_c, op, xs)
                assert np.isfinite(want).all() == (case == "finite"), (case, op, want)
                U.assert_same_class_bits(got, want, f"{path} n={n} {case} {op} on {where} [{log}]")
        return
    for i, (op, fam) in enumerate(REDUCE_OPS):
        region = SCRATCH.get("reduce:" + rc.leaf(op, leaf))
        if i == 0:
            _first_call_recorded(inst, lambda: rc.call(op), region, f"{path} n={n} {op}")
        cases = _reduce_cases(n, off, dtype, fam)
        rc.write(rc.xs(cases[0][1]))
        rc.call(op)
        eager = inst.take_path()
        assert rc.leaf(op, leaf) in eager, (path, n, op, eager)
        rec, log = _record(inst, lambda: rc.call(op))
        try:
            assert log == eager, f"{path} n={n} {op}: recorded {log!r}, eager {eager!r}"
            order = cases + cases[:1]  # (every case, then the first again)
            for j, (case, x) in enumerate(order):
                xs = rc.xs(x)
                rc.write(xs)
                rec.submit()
                got = rc.res.read(inst.device())
                want = rc.want(oracle_c, op, xs)
                assert np.isfinite(want).all() == (case == "finite"), (case, op, want)
                U.assert_same_class_bits(got, want, f"{path} n={n} {op} replay {j} ({case}) [{log}]")
            if i == 2:  # (Sum: other rows' workspace traffic and a regrow, then one more replay)
                canaries = _intrude(inst)
                xs = rc.xs(cases[1][1])
                rc.write(xs)
                rec.submit()
                U.assert_same_class_bits(rc.res.read(inst.device()), rc.want(oracle_c, op, xs), f"{path} n={n} {op} replay after the regrow [{log}]")
                _check_canaries(inst, canaries, f"{path} n={n}")
        finally:
            rec.destroy()


# --------------------------------------------------------------------------------------------------------
# Gemv + Reduce (wg_gemv_reduce): the fused kernel's arrival counter and y in the transpose workspace
# --------------------------------------------------------------------------------------------------------
GEMV_REDUCE_SHAPES = [(512, 256, "gemv.small_reduce/rl=2"), (2048, 512, "gemv.small_reduce/rl=4"), (4096, 1024, "gemv.small_reduce/rl=8"),
                      (8192, 1024, "gemv_reduce.two>gemv>")]
GEMV_REDUCE_PARAMS = [pytest.param(R, C, leaf, w, id=f"{R}x{C}-{w}") for R, C, leaf in GEMV_REDUCE_SHAPES for w in WHERE]


def _gemv_reduce_want(oracle_c, A, V, op):
    from oracle import wgsl_oracle as wo
    y = U.special_product(A, V, F32)[:, 0, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array([oracle_c.reduce(int(getattr(wo, op.upper())), y, wo.Shape(y.size, 1, 1, y.size, y.size, 0))], np.float32)


@pytest.mark.parametrize("R,C,leaf,where", GEMV_REDUCE_PARAMS)
def test_gemv_reduce_in_context(request, masked, oracle_c, R, C, leaf, where):
    """Every case of GEMV_REDUCE_CASES (finite, overflow, +Inf with -Inf, one -Inf, NaN) and each of its ops; replayed: one recording per op, submitted
    on every case in turn and on the first again -- the fused kernel must have set its arrival counter back to 0 after each launch."""
    wg = _wg()
    inst = request.getfixturevalue("fresh") if where == "replay" else masked(where)
    rng = np.random.default_rng(R + C)
    data = {case: _gemv_reduce_operands(rng, R, C, case) for case in GEMV_REDUCE_CASES}
    A0, V0 = data["finite"]
    m = Stored(inst, A0, F32, "aligned")
    v = _upload(inst, V0.ravel().astype(F32))
    res = _upload(inst, np.full(1, np.nan, F32))
    mv = wg.GpuTensorView(m.cm, m.buf, 2)

    def call(op):
        enc = inst.device().create_command_encoder()
        with enc.compute_pass("gemv_reduce", None) as p:
            wg.gemv_reduce(p, wg.ReduceOp[op], res, mv, v, wg.GemvVariant.Gemv)

    def put(case):
        A, V = data[case]
        _write(inst, m, A)
        inst.queue().write_buffer(v, 0, V.ravel().astype(F32))
        inst.queue().write_buffer(res, 0, np.full(1, np.nan, F32))

    def check(case, op, log, what):
        want = _gemv_reduce_want(oracle_c, *data[case], op)
        assert _klass(want[0]) == GEMV_REDUCE_CASES[case][op], (case, op, want)
        U.assert_same_class_bits(res.read(inst.device()), want, f"gemv_reduce {R} x {C} {case} {op} {what} [{log}]")

    if where != "replay":
        for case, ops in GEMV_REDUCE_CASES.items():
            for op in ops:
                put(case)
                inst.take_path()
                call(op)
                log = inst.take_path()
                _assert_leaf(log, where, f"gemv_reduce:{R}x{C}", leaf, what=f"gemv_reduce {R} x {C} {op}")
                check(case, op, log, f"on {where}")
        return
    _first_call_recorded(inst, lambda: call("Sum"), SCRATCH.get("gemv_reduce:" + leaf), f"gemv_reduce {R} x {C}")
    if leaf.startswith("gemv.small_reduce"):  # y's region sized by a two-launch call (GemvTr: never fused), the counter still missing: only it can fail
        mt, v4 = Stored(inst, np.ones((4, R, 1)), F32, "dense"), _upload(inst, np.ones(4, F32))
        enc = inst.device().create_command_encoder()
        with enc.compute_pass("gemv_reduce", None) as p:
            wg.gemv_reduce(p, wg.ReduceOp.Sum, res, wg.GpuTensorView(mt.cm, mt.buf, 2), v4, wg.GemvVariant.GemvTr)
        assert "gemv_reduce.two>" in inst.take_path()
        _first_call_recorded(inst, lambda: call("Sum"), "arrival counter", f"gemv_reduce {R} x {C} (counter)")
    for i, op in enumerate(("Min", "Max", "Sum", "SqNorm", "Prod")):
        cases = [c for c, ops in GEMV_REDUCE_CASES.items() if op in ops]
        put(cases[0])
        call(op)
        eager = inst.take_path()
        assert leaf in eager, (R, C, op, eager)
        rec, log = _record(inst, lambda: call(op))
        try:
            assert log == eager, f"{R} x {C} {op}: recorded {log!r}, eager {eager!r}"
            for j, case in enumerate(cases + cases[:1]):
                put(case)
                rec.submit()
                check(case, op, log, f"replay {j}")
            if i == 2:
                canaries = _intrude(inst)
                put(cases[1])
                rec.submit()
                check(cases[1], op, log, "replay after the regrow")
                _check_canaries(inst, canaries, f"gemv_reduce {R} x {C}")
        finally:
            rec.destroy()


# --------------------------------------------------------------------------------------------------------
# the guard: the masked contexts really do move leaves
# --------------------------------------------------------------------------------------------------------
def test_masked_contexts_move_leaves():
    """Each masked context has rows whose split count or leaf differs from the full chip's (CTX_LEAF; each of those rows asserts it reaches that tag and
    not the full chip's). If the heuristics stopped reading the CU count, those rows would fail; this keeps the table from quietly emptying."""
    for where in MASKED:
        moved = {k[1] for k in CTX_LEAF if k[0] == where}
        assert len(moved) >= 5, f"{where}: only {len(moved)} rows reach another leaf than on the full chip"
