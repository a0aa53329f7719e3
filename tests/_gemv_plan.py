"""What the Gemv front-end (wgmath_amd/csrc/api.hip: wg_gemv, wg_gemv_mixed, wg_gemv_reduce) hands to which launcher, and that launcher's planner through the C ABI
(wg_debug_gemv_plan, wg_debug_gemv_any_plan). Shared by tests/golden/make_gemv_plan_golden.py, tests/test_gemv_plan_host.py and tests/test_gpu_gemv_plan.py."""
import ctypes

# one row of tests/golden/gemv_plan_parent.json: `kind`, the 19 query fields, then what was recorded
QUERY = ("trans", "rows_out", "k", "nrhs", "nmats", "m_elem", "v_elem", "bf16", "gemm16", "ldm", "ldv", "ldo", "m_batch", "v_batch", "o_batch", "m_addr16", "v_addr16",
         "cus", "gemvt_lds")
FIELDS = ("kind",) + QUERY + ("status", "log", "src", "ret")
# kind: the launcher the front-end calls with the query
K_GEMV, K_ANY, K_REDUCE = 0, 1, 2  # wgk_gemv / wgk_gemv_mixed; wgk_gemv_any / _any_mixed; wg_gemv_reduce's fused-or-two-launches choice (the query is the Gemv's)
ELEMS = {"f32": (4, 4, 0, 0), "f16": (2, 2, 0, 1), "bf16": (2, 2, 1, 1), "f16w": (2, 4, 0, 0), "bf16w": (2, 4, 1, 0)}  # m_elem, v_elem, bf16, gemm16


def vec4_ok(rows, cols, mats, off, ld, batch):
    """api.hip vec4_ok: a view the 16-byte kernels address as it is."""
    return not (rows % 4 or off % 4 or (cols > 1 and ld % 4) or (mats > 1 and batch % 4))


def up8(x):
    return (x + 7) & ~7


def query(lib, **kw):
    q = lib.GemvQueryC()
    for k, v in kw.items():
        assert k in QUERY, k
        setattr(q, k, int(v))
    return q


def route(lib, elems, tr, R, C, nrhs, mats, m, v, o, base16=(0, 0), cus=256, gemvt_lds=0):
    """A wg_gemv (elems f32 / f16 / bf16) or wg_gemv_mixed (f16w / bf16w) call on an R x C matrix as stored, with views m, v, o = (offset, leading dimension,
    matrix stride) in elements and the two read buffers' base addresses modulo 16: (kind, wrapper tag, query) as api.hip decides -- the vec4 kernels on the views
    as they are, on staged copies of vectors / result that are off ("stage>"), or the any-alignment kernels for a matrix that is off; None: no launch."""
    m_elem, v_elem, bf16, gemm16 = ELEMS[elems]
    rows_out, k = (C, R) if tr else (R, C)
    if rows_out == 0 or nrhs == 0 or mats == 0:
        return None
    m_ok = vec4_ok(R, C, mats, *m) and rows_out % 4 == 0 and k % 4 == 0
    v_ok, o_ok = vec4_ok(k, nrhs, mats, *v), vec4_ok(rows_out, nrhs, mats, *o)
    common = dict(trans=tr, rows_out=rows_out, k=k, nrhs=nrhs, nmats=mats, m_elem=m_elem, v_elem=v_elem, bf16=bf16, gemm16=gemm16, cus=cus, gemvt_lds=gemvt_lds)
    if not m_ok:  # one pass over the matrix where it lies (the planner of gemv_any reads no stride and no address)
        return None if k == 0 else (K_ANY, "", query(lib, **common))
    (mo, ldm, mb), (vo, ldv, vb), (_, ldo, ob) = m, v, o
    m16, v16 = (base16[0] + mo * m_elem) % 16, (base16[1] + vo * v_elem) % 16
    if not v_ok:  # a dense copy at the start of the staging workspace
        ldv, vb, v16 = k, k * nrhs, 0
    if not o_ok:
        ldo, ob = rows_out, rows_out * nrhs
    return (K_GEMV, "" if v_ok and o_ok else "stage>",
            query(lib, ldm=ldm, ldv=ldv, ldo=ldo, m_batch=mb, v_batch=vb, o_batch=ob, m_addr16=m16, v_addr16=v16, **common))


def plan(lib, q):
    """(plan, tags) of wg_debug_gemv_plan."""
    p, buf = lib.GemvPlanC(), ctypes.create_string_buffer(256)
    lib.check(lib.lib.wg_debug_gemv_plan(ctypes.byref(q), ctypes.byref(p), buf, len(buf)))
    return p, buf.value.decode()


def any_plan(lib, q):
    p, buf = lib.GemvAnyPlanC(), ctypes.create_string_buffer(96)
    lib.check(lib.lib.wg_debug_gemv_any_plan(ctypes.byref(q), ctypes.byref(p), buf, len(buf)))
    return p, buf.value.decode()


def fused_reduce(lib, q):
    """wg_gemv_reduce runs ONE launch exactly when the plan of its Gemv -- one matrix, one right-hand side -- is the single-kernel leaf."""
    q1 = lib.GemvQueryC.from_buffer_copy(q)
    q1.nrhs = q1.nmats = 1
    return lib.GEMV_LEAVES[plan(lib, q1)[0].leaf] == "small"


def planned(lib, kind, q):
    """(status, log) the planner states for a row of `kind`: what the call returns and what wg_debug_take_path holds after it, behind a "stage>" wrapper if there is
    one -- for K_REDUCE up to the Reduce launch's own tag."""
    if kind == K_ANY:
        p, log = any_plan(lib, q)
        return p.status, log
    p, log = plan(lib, q)
    status = p.status if lib.GEMV_LEAVES[p.leaf] in ("nothing", "unsupported") else 0
    if kind == K_REDUCE:
        if fused_reduce(lib, q):
            return 0, f"gemv.small_reduce/rl={p.rl}"
        return status, "gemv_reduce.two>" + log
    return status, log
