"""Shared by tests/golden/make_quant_plan_golden.py (which records) and tests/test_quant_plan_parent.py (which compares): the queries that pin the five quantized
planners -- wg_debug_{gemv_q8,gemv_q4,gemm_q8,gemm_q4,gemm_q8a8}_plan -- to the commit before they were given one shared core. Nothing here needs a device.

Two kinds of queries per family:
  explicit(family)   200 to 250 queries, named by their construction: the cut cases of the GPU tests on 256, 16 and 8 CUs, and both sides of every threshold the planners
                     have. The golden file stores each with every plan field, the status, the message and the tags.
  block(family, b)   BLOCKS blocks of BLOCK_SIZE queries from the integer generator below (a 64-bit LCG: no library's random stream is involved): fields drawn from
                     the same edge values, perturbed. The golden file stores one SHA-256 per block.
"""
import ctypes
import hashlib

from wgmath_amd import _lib as L

BLOCKS, BLOCK_SIZE = 100, 1000
U32 = 0xffffffff
WHOLE = 1 << 30

FAMILIES = {  # name -> (query struct, plan struct); the entry point is wg_debug_<name>_plan
    "gemv_q8": (L.GemvQ8QueryC, L.GemvQ8PlanC),
    "gemv_q4": (L.GemvQ4QueryC, L.GemvQ4PlanC),
    "gemm_q8": (L.GemmQ8QueryC, L.GemmQ8PlanC),
    "gemm_q4": (L.GemmQ4QueryC, L.GemmQ4PlanC),
    "gemm_q8a8": (L.GemmQ8A8QueryC, L.GemmQ8A8PlanC),
}
TAGS_CAP = 128


def query_fields(fam):
    return [n for n, _ in FAMILIES[fam][0]._fields_]


def plan_fields(fam):
    """The plan's numeric fields in struct order, `grid` as three; status and message are stored beside them."""
    out = []
    for n, _ in FAMILIES[fam][1]._fields_:
        if n in ("status", "message"):
            continue
        out += ["grid0", "grid1", "grid2"] if n == "grid" else [n]
    return out


def bind(lib):
    """The five entry points of `lib` (a ctypes.CDLL of any build of the library) with their signatures."""
    fns = {}
    for fam, (Q, P) in FAMILIES.items():
        fn = getattr(lib, f"wg_debug_{fam}_plan")
        fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(Q), ctypes.POINTER(P), ctypes.c_char_p, ctypes.c_size_t]
        fns[fam] = fn
    return fns


def _numeric_ranges(P):
    """Byte ranges of the plan struct that hold its numeric fields and the status: everything but the message and the padding."""
    ranges = []
    for n, t in P._fields_:
        if n == "message":
            continue
        d = getattr(P, n)
        if ranges and ranges[-1][1] == d.offset:
            ranges[-1][1] = d.offset + d.size
        else:
            ranges.append([d.offset, d.offset + d.size])
    return [tuple(r) for r in ranges]


class Runner:
    """Asks one family's planner of one library."""

    def __init__(self, fns, fam):
        self.fam, self.fn = fam, fns[fam]
        self.Q, self.P = FAMILIES[fam]
        self.plan, self.tags = self.P(), ctypes.create_string_buffer(TAGS_CAP)
        self.ranges = _numeric_ranges(self.P)
        self.msg_off = self.P.message.offset

    def _call(self, values):
        rc = self.fn(ctypes.byref(self.Q(*values)), ctypes.byref(self.plan), self.tags, TAGS_CAP)
        assert rc == 0, (self.fam, values, rc)

    def row(self, values):
        """[plan fields ..., status, message, tags] of the query `values` (in the query struct's field order)."""
        self._call(values)
        p, out = self.plan, []
        for n, _ in self.P._fields_:
            if n in ("status", "message"):
                continue
            out += list(p.grid) if n == "grid" else [getattr(p, n)]
        return out + [p.status, p.message.decode(), self.tags.value.decode()]

    def digest(self, queries):
        """SHA-256 over the queries' concatenated (plan bytes without padding, status, message, tags)."""
        h = hashlib.sha256()
        for values in queries:
            self._call(values)
            raw = bytes(self.plan)
            for a, b in self.ranges:
                h.update(raw[a:b])
            h.update(raw[self.msg_off:self.msg_off + 128].split(b"\0")[0] + b"\0" + self.tags.value + b"\0")
        return h.hexdigest()


# ---- the explicit queries --------------------------------------------------------------------------------------------------------------------------------
def _values(fam, kw):
    fields = FAMILIES[fam][0]._fields_
    assert set(kw) <= {n for n, _ in fields}, set(kw) - {n for n, _ in fields}
    return tuple(int(kw.get(n, 0)) & (U32 if t is ctypes.c_uint32 else 0xffffffffffffffff) for n, t in fields)


def _gemm(fam, k, outs, n, mats=1, G=32, Gx=None, cus=256, bf16=0, **over):
    """An aligned dense call of a Gemm family; `over` replaces single fields afterwards (a misalignment on its own). k: logical rows; q4's ldm counts bytes."""
    ldm = k // 2 if fam == "gemm_q4" else k
    kw = dict(k=k, outputs=outs, n=n, mats=mats, group_rows=G, ldm=ldm, lds=max(-(-k // G), 1), ldx=k, ldo=outs, m_batch=ldm * outs, s_batch=max(-(-k // G), 1) * outs,
              x_batch=k * n, o_batch=outs * n, m_addr16=0, x_addr16=0, o_addr16=0, cus=cus)
    if fam == "gemm_q8a8":
        gx = G if Gx is None else Gx
        kw.update(x_group_rows=gx, ldxs=max(-(-k // gx), 1), xs_batch=max(-(-k // gx), 1) * n)
    else:
        kw["x_bf16"] = bf16
    kw.update(over)
    return kw


def _gemm_explicit(fam):
    import _gemm_q4, _gemm_q8, _gemm_q8a8
    H = {"gemm_q8": _gemm_q8, "gemm_q4": _gemm_q4, "gemm_q8a8": _gemm_q8a8}[fam]
    a8 = fam == "gemm_q8a8"
    out = []
    # the cut cases of the GPU tests, the lane-map cut and the call that dirties the workspace: 256, 16 and 8 CUs (bf16: three of them -- the tag alone differs)
    for i, c in enumerate(H.CUT_CASES + [H.CUT_LANE_MAP, H.DIRTY]):
        for cus in (256, 16, 8):
            out.append(H.query_kw(c, cus=cus) if a8 else H.query_kw(c, "f16", cus=cus))
        if not a8:
            out.append(H.query_kw(c, "bf16", cus=256))

    def add(*a, **kw):
        out.append(_gemm(fam, *a, **kw))

    # the column tile and the passes: n at 32 / 33, 64 / 65, 65535 / 65536 (the combine pass puts n on grid.y: no cut from 65536 on)
    for n in (1, 31, 32, 33, 63, 64, 65, 128, 129, 65535, 65536):
        add(4096, 16, n)
        if n in (32, 33, 64, 65):
            add(4096, 4096, n)
    add(65536, 16, 65535, cus=8)
    add(65536, 16, 65536, cus=8)
    # grid.z: matrices x column passes at 65535 / 65536, and the matrices alone on the element-by-element kernel
    for mats, n in ((65535, 64), (65536, 64), (65535, 1), (21845, 129), (21846, 129), (32767, 65), (32768, 65), (1, 65535 * 64), (1, 65535 * 64 + 1), (0, 16)):
        add(1024, 16, n, mats=mats)
    for mats in (65535, 65536):
        add(1024, 16, 3, mats=mats, m_addr16=1)
    # k: one step either side of the floor of a split (512), of two floors (1024), of the next ones; no whole step; nothing
    for k in (0, 16, 32, 48, 480, 512, 544, 992, 1024, 1056, 1088, 1536, 2016, 2048, 2080, 4096):
        add(k, 16, 16)
        if k >= 480:
            add(k, 16, 16, G=WHOLE)
    # group_rows: the step, three steps, no multiple of the step, k, beyond k
    for k in (1120, 4096):
        for G in (32, 48, 96, 544, k, k + 1) if k == 1120 else (16, 32, 48, 96, 1024, 1536, k - 32, k, k + 1, U32):
            add(k, 33, 20, G=G)
            if a8 and k == 4096 and G in (16, 48, 96, 1024, k, k + 1):
                add(k, 33, 20, G=32, Gx=G)
    if a8:  # both orders of the two group sizes; the chain cap as the unit where neither side has groups
        for G, Gx in ((64, 128), (128, 64), (32, WHOLE), (WHOLE, 32), (WHOLE, WHOLE), (1536, WHOLE), (WHOLE, 1536), (WHOLE, 2048), (2048, WHOLE), (48, 32), (32, 48),
                      (96, 192), (192, 96), (1024, 2048), (2048, 1024)):
            add(3072, 33, 20, G=G, Gx=Gx)
            if WHOLE in (G, Gx):
                add(8192, 33, 20, G=G, Gx=Gx)
    # every address, leading dimension and matrix stride misaligned on its own -- where it counts (several outputs / columns / matrices) and where it does not
    xa = 16 if a8 else 8  # elements of x in 16 bytes
    for over in (dict(m_addr16=1), dict(m_addr16=8), dict(x_addr16=2), dict(x_addr16=8), dict(o_addr16=4), dict(ldm=2048 + 8), dict(ldx=2048 + xa // 2),
                 dict(ldx=2048 + xa), dict(ldx=2048 + 8), dict(ldo=33 + 1), dict(lds=77), dict(m_batch=2048 * 33 + 8), dict(x_batch=2048 * 20 + xa // 2),
                 dict(x_batch=2048 * 20 + 8), dict(o_batch=33 * 20 + 1), dict(s_batch=7)):
        if fam == "gemm_q4" and "ldm" in over:
            over = dict(ldm=1024 + 8)
        if fam == "gemm_q4" and "m_batch" in over:
            over = dict(m_batch=1024 * 33 + 8)
        add(2048, 33, 20, mats=2, **over)
        if "batch" in list(over)[0] or list(over)[0] in ("m_addr16", "ldm"):
            add(2048, 33, 20, **over)  # (one matrix: the strides between matrices are never used)
    add(2048, 1, 20, ldm=(1024 if fam == "gemm_q4" else 2048) + 8)  # one output: ldm is never used
    add(2048, 33, 1, ldx=2048 + 4)                                   # one column: ldx is never used
    if a8:
        add(2048, 33, 20, ldxs=99)
        add(2048, 33, 20, mats=2, xs_batch=5)
    # the CU count: none reported, masked contexts, the whole chip, more
    for cus in (0, 1, 8, 16, 100, 248, 256, 304, U32):
        add(4096, 130, 130, mats=2, cus=cus)
        add(65536, 16, 16, G=WHOLE, cus=cus)
    # k and outputs within 64 of 2^32
    for k in (U32 - 63, U32 - 31, U32 - 16, U32):
        for G in (32, WHOLE):
            add(k, 16, 16, G=G)
        add(k, 16, 16, G=WHOLE, cus=8)
    for outs in (U32 - 64, U32 - 63, U32 - 1, U32):
        add(4096, outs, 16)
        add(32, outs, 65)
    add(48, U32, 3)
    add(U32 - 31, U32, 65536, G=WHOLE)
    # more splits wanted than grid.y holds: the clamp to 65535 (k = 65535 * 65536: one split fewer and the rows per split pass a multiple of every unit)
    for cus in (1 << 20, U32):
        add(0xffff0000, 16, 16, G=U32, cus=cus)  # (one group per output)
    if not a8:
        add(4096, 16, 16, bf16=1)
    return out


def _gemv(fam, tr, R, C, nrhs=1, mats=1, G=32, cus=256, **over):
    """An aligned dense call of a Gemv family on a stored R x C matrix (gemv_q4: R rows of BYTES, k = 2 R)."""
    k, outs = (R, C) if tr else (C, R)
    kk = 2 * k if fam == "gemv_q4" else k
    kw = dict(trans=int(tr), rows=R, cols=C, nrhs=nrhs, mats=mats, group_rows=G, cus=cus, ldm=R, lds=max(-(-kk // G), 1), ldv=kk, ldo=outs, m_batch=R * C,
              s_batch=max(-(-kk // G), 1) * C, v_batch=kk * nrhs, o_batch=outs * nrhs, m_addr16=0, v_addr16=0)
    if fam == "gemv_q8":
        kw["o_addr16"] = 0
    kw.update(over)
    return kw


def _gemv_explicit(fam):
    q8 = fam == "gemv_q8"
    if q8:
        import _q8 as H
    else:
        import _q4 as H

    def case_query(case, cus):
        """The query a call on the views the GPU test builds for a row of H.CASES fills (gemv_q4's rows have no variant and give k in logical rows)."""
        name, tr, R, C, nrhs, Z, G, (moff, mpad, gap), voff, tag = case if q8 else case[:1] + (True, case[1] // 2) + case[2:]
        k, outs = (R, C) if tr else (C, R)
        kk, pad = (k if q8 else 2 * k), (4 if voff else 0)
        grows = R if q8 else 2 * R  # the groups run along the stored rows
        kw = dict(trans=int(tr), rows=R, cols=C, nrhs=nrhs, mats=Z, group_rows=G, cus=cus, ldm=R + mpad, m_batch=(R + mpad) * C + gap, m_addr16=moff % 16,
                  lds=-(-grows // G), s_batch=-(-grows // G) * C, ldv=kk + pad, v_batch=(kk + pad) * nrhs, v_addr16=4 * voff % 16, ldo=outs + pad, o_batch=(outs + pad) * nrhs)
        if q8:
            kw["o_addr16"] = 4 * voff % 16
        return kw

    # the cut cases of the GPU tests (the rows named *_split) and the call that dirties the workspace: 256, 16 and 8 CUs; gemv_q4's other cases too
    out = [case_query(c, cus) for c in H.CASES + [H.DIRTY] if c[0].endswith("_split") or c is H.DIRTY or not q8 for cus in (256, 16, 8)]

    def add(*a, **kw):
        out.append(_gemv(fam, *a, **kw))

    trs = (True, False) if q8 else (True,)
    chunk = 512  # rows of the stored matrix a half-wave covers per load (gemv_q4: bytes)
    # the register tile and the groups of right-hand sides; 65535 / 65536 of them (the combine pass puts them on grid.y)
    for tr in trs:
        for nrhs in (0, 1, 2, 3, 4, 5, 8, 9, 65535, 65536):
            add(tr, 65536 if tr else 16, 8 if tr else 65536, nrhs)
            if nrhs in (3, 9):
                add(tr, 1024, 4096, nrhs)
        # grid.z: matrices x groups of 8 right-hand sides at 65535 / 65536
        for mats, nrhs in ((65535, 8), (65536, 8), (65536, 1), (32767, 9), (32768, 9), (21845, 17), (21846, 17), (1, 8 * 65535), (1, 8 * 65535 + 1), (0, 1)):
            add(tr, 512, 8, nrhs, mats=mats)
            if nrhs == 8:
                add(tr, 512, 8, nrhs, mats=mats, m_addr16=1)
    # T: the contraction one chunk and one piece either side of the floor (8 chunks), of two and three floors; no whole piece; nothing
    for R in (0, 16, 37, 512, 8 * chunk - chunk, 8 * chunk - 16, 8 * chunk, 8 * chunk + 16, 16 * chunk - chunk, 16 * chunk - 16, 16 * chunk, 16 * chunk + 16,
              24 * chunk - 16, 24 * chunk, 65536 + 16):
        add(True, R, 8)
        if R >= 7 * chunk:
            add(True, R, 9, 3)
        if R in (8 * chunk, 16 * chunk - 16, 16 * chunk):
            add(True, R, 4096)
    # T: 4 columns per half-wave where 32 columns per workgroup still give every CU a workgroup
    for C in (0, 1, 32, 33, 4064, 4096, 8160, 8192, 8193):
        for R, cus in ((4096, 256), (8192, 128)):
            add(True, R, C, cus=cus)
        if C in (4064, 4096):
            add(True, 4096, C, 8)
    if q8:  # N: the contraction (columns) one piece either side of the floor (64) and its multiples; rows around a workgroup's 1024
        for C in (0, 48, 64, 80, 112, 128, 144, 65537):
            add(False, 16, C)
            if C in (64, 128):
                add(False, 16, C, 3, cus=8)
        for R in (0, 37, 1024, 1040):
            add(False, R, 4096)
        add(False, 1040, 64)
    else:
        add(False, 4096, 8)                # wg_gemv_q4 computes W^T v only
        add(False, 0, 0)
        for R in (0x7fffffe0, 0x7ffffff0, 0x7fffffff, 0x80000000, 0x80000010, U32):  # k = 2 rows must fit 32 bits
            add(True, R, 8)
            add(True, R, 8, cus=8)
    # group_rows does not enter the plan; the step, three steps, no multiple, k, beyond k
    for G in (16, 48, 8192, 8193, U32):
        for tr in trs:
            add(tr, 8192, 8, G=G)
    # every address, leading dimension and matrix stride misaligned on its own -- where it counts and where it does not
    for tr in trs:
        R, C = (8192, 9) if tr else (1040, 192)
        k, outs = (R, C) if tr else (C, R)
        kk = k if q8 else 2 * k
        overs = [dict(m_addr16=1), dict(m_addr16=8), dict(v_addr16=4), dict(v_addr16=8), dict(ldm=R + 8), dict(ldm=R + 3), dict(ldv=kk + 2), dict(ldv=kk + 4),
                 dict(ldo=outs + 2), dict(lds=99), dict(m_batch=R * C + 8), dict(v_batch=kk * 2 + 2), dict(v_batch=kk * 2 + 4), dict(o_batch=outs * 2 + 2),
                 dict(s_batch=7)]
        if q8:
            overs += [dict(o_addr16=4), dict(o_addr16=8)]
        for over in overs:
            add(tr, R, C, 2, mats=2, **over)
            if tr and list(over)[0] not in ("m_addr16", "v_addr16", "o_addr16", "lds", "s_batch"):
                add(tr, R, C, **over)  # (one right-hand side, one matrix: the strides are never used)
    add(True, 8192, 1, ldm=8192 + 8)  # one column: ldm is never used
    # the CU count: none reported, masked contexts, the whole chip, more
    for cus in (0, 1, 8, 16, 100, 248, 256, 304, U32):
        for tr in trs:
            add(tr, 65536 if tr else 1024, 8 if tr else 65536, cus=cus)
            if tr and cus in (0, 8, 16, 256):
                add(tr, 8192, 4096, 2, mats=2, cus=cus)
    # k and the outputs within 64 of 2^32 (gemv_q4: of 2^31 rows of bytes, above)
    for big in (U32 - 63, U32 - 15, U32):
        if q8:
            for tr in trs:
                add(tr, big, 8)
                if not tr:
                    add(tr, 16, big)
                if big == U32 - 63:
                    add(tr, big, 8, cus=8)
        else:
            add(True, 4096, big)
            add(True, 16, big, cus=8)
    # more splits wanted than grid.y holds: the clamp to 65535 (k = 65535 * 65536: one split fewer and the rows per split pass a multiple of every unit)
    for cus in (1 << 20, U32):
        add(True, 0xffff0000 if q8 else 0x7fff8000, 8, cus=cus)
        if q8:
            add(False, 16, 0xffff0000, cus=cus)
    return out


def explicit(fam):
    """The explicit queries of a family, as value tuples in the query struct's field order, without repeats."""
    kws = _gemm_explicit(fam) if fam.startswith("gemm") else _gemv_explicit(fam)
    seen, out = set(), []
    for kw in kws:
        v = _values(fam, kw)
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# ---- the generated blocks --------------------------------------------------------------------------------------------------------------------------------
class Lcg:
    """x <- x * 6364136223846793005 + 1442695040888963407 (mod 2^64); a draw is the high 32 bits."""

    def __init__(self, seed):
        self.x = seed & 0xffffffffffffffff

    def __call__(self):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & 0xffffffffffffffff
        return self.x >> 32


def _pick(r, edges, steps):
    """An edge value chosen by the low bits of the draw r; three times in eight moved by +- one of `steps` (clamped to 32 bits)."""
    v = edges[(r & 0xffff) % len(edges)]
    s = (r >> 16) & 7
    if s >= 5:
        d = steps[(r >> 19) % len(steps)]
        v = v - d if (r >> 27) & 1 else v + d
    return 0 if v < 0 else U32 if v > U32 else v


_K = (0, 32, 480, 512, 544, 992, 1024, 1056, 1088, 1120, 1536, 2048, 2560, 3072, 4096, 8192, 11008, 16384, 16896, 18432, 29696, 65536, 131104, 1 << 20, 0xffff0000, U32 - 63, U32 - 31)
_OUTS = (0, 1, 7, 8, 9, 16, 17, 32, 33, 64, 127, 128, 129, 130, 256, 1024, 2048, 4064, 4096, 8192, 8193, 11008, 65536, U32 - 64, U32)
_N = (0, 1, 2, 3, 8, 9, 16, 20, 31, 32, 33, 64, 65, 128, 130, 192, 65535, 65536)
_MATS = (1, 1, 1, 1, 1, 1, 2, 2, 3, 5, 0, 1023, 8191, 21845, 21846, 32767, 32768, 65535, 65536)
_CUS = (0, 1, 8, 16, 64, 100, 128, 248, 256, 256, 256, 304, 1 << 20, U32)
_G = (16, 32, 32, 48, 64, 96, 128, 256, 512, 544, 1024, 1536, 2048, 4096, WHOLE, U32)
_PAD = (0, 0, 0, 0, 16, 32, 48, 8, 4, 3, 1, 2)
_A16 = (0, 0, 0, 0, 0, 0, 1, 2, 4, 8, 12, 15)


def _views(r):
    """Six paddings / offsets from one draw: most queries are aligned in everything (three in four), the others draw each from _PAD / _A16."""
    if r & 3:
        return (0, 0, 0, 0, 0, 0)
    r >>= 2
    return (_PAD[r % 12], _PAD[(r >> 4) % 12], _PAD[(r >> 8) % 12], _PAD[(r >> 12) % 12], _A16[(r >> 16) % 12], _A16[(r >> 20) % 12])


def _gemm_random(fam, rnd):
    k = _pick(rnd(), _K, (32, 16, 1, 64, 512))
    outs = _pick(rnd(), _OUTS, (1, 32, 63))
    n = _pick(rnd(), _N, (1,))
    r = rnd()
    mats, cus = _MATS[(r & 0xffff) % len(_MATS)], _CUS[(r >> 16) % len(_CUS)]
    r = rnd()
    G = (k, k + 1, max(k, 32) - 32)[(r >> 8) % 3] if r & 7 == 0 else _G[(r >> 8) % len(_G)]
    Gx = G if r & 0x30 == 0 else (k, k + 1, 2 * G, max(G // 2, 1))[(r >> 16) % 4] if r & 0x40 else _G[(r >> 16) % len(_G)]
    G, Gx = G & U32 or 1, Gx & U32 or 1
    pm, px, pmb, pxb, am, ax = _views(rnd())
    ldm = ((k // 2 if fam == "gemm_q4" else k) + pm) & U32
    ldx = (k + px) & U32
    lds = -(-k // G) or 1
    kw = dict(k=k, outputs=outs, n=n, mats=mats, group_rows=G, ldm=ldm, lds=lds, ldx=ldx, ldo=outs, m_batch=ldm * outs + pmb, s_batch=lds * outs, x_batch=ldx * n + pxb,
              o_batch=outs * n, m_addr16=am, x_addr16=ax, o_addr16=(r >> 24) & 12, cus=cus)
    if fam == "gemm_q8a8":
        ldxs = -(-k // Gx) or 1
        kw.update(x_group_rows=Gx, ldxs=ldxs, xs_batch=ldxs * n)
    else:
        kw["x_bf16"] = (r >> 28) & 1
    return kw


_ROWS = (0, 16, 32, 37, 496, 512, 528, 1024, 1040, 2048, 3584, 4080, 4096, 4112, 4608, 5168, 7680, 8192, 8704, 12288, 16384, 65536, 1 << 20, 0x7fff8000, 0x7ffffff0, 0x80000000,
         0xffff0000, U32 - 63, U32 - 15)
_NCOLS = (0, 1, 7, 8, 9, 16, 31, 32, 33, 48, 64, 80, 128, 192, 255, 320, 1024, 2048, 4064, 4096, 8192, 8193, 65536, 0xffff0000, U32 - 63, U32)
_NRHS = (0, 1, 1, 1, 2, 2, 3, 4, 5, 8, 9, 11, 16, 17, 65535, 65536)


def _gemv_random(fam, rnd):
    q8 = fam == "gemv_q8"
    R = _pick(rnd(), _ROWS, (16, 512, 1, 32))
    C = _pick(rnd(), _NCOLS, (1, 16, 32))
    r = rnd()
    nrhs, mats, cus = _NRHS[(r & 0xff) % len(_NRHS)], _MATS[(r >> 8 & 0xff) % len(_MATS)], _CUS[(r >> 16 & 0xff) % len(_CUS)]
    tr = (r >> 24) & 1 if q8 else int((r >> 24) & 15 != 0)
    G = _G[(r >> 28) % len(_G)]
    k, outs = (R, C) if tr else (C, R)
    kk = k if q8 else (2 * k) & U32
    pm, pv, pmb, pvb, am, av = _views(rnd())
    ldm, ldv, ldo = (R + pm) & U32, (kk + pv) & U32, (outs + (pv >> 1)) & U32
    lds = -(-kk // G) or 1
    kw = dict(trans=tr, rows=R, cols=C, nrhs=nrhs, mats=mats, group_rows=G, cus=cus, ldm=ldm, lds=lds, ldv=ldv, ldo=ldo, m_batch=ldm * C + pmb, s_batch=lds * C,
              v_batch=ldv * nrhs + pvb, o_batch=ldo * nrhs + (pvb >> 1), m_addr16=am, v_addr16=av)
    if q8:
        kw["o_addr16"] = av if pvb else 0
    return kw


def block(fam, b):
    """Block b of a family: BLOCK_SIZE queries as value tuples."""
    rnd = Lcg((list(FAMILIES).index(fam) + 1) * 0x9e3779b97f4a7c15 + b * 0xd1342543de82ef95 + 1)
    make = _gemm_random if fam.startswith("gemm") else _gemv_random
    return [_values(fam, make(fam, rnd)) for _ in range(BLOCK_SIZE)]
