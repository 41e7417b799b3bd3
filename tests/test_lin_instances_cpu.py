"""CPU: the linear instance table (tests/lin_instances.py) names the kernel the planner picks for each row (qe_quantlinear_form,
qe_quantlinear_float_input_path: host-only queries), and together its rows reach every instance the linear launchers can
select: 20 int8 MFMA instances (four kernels x F32 / CODES / CODES_GELU / RES / BF16), both linear_f32_mfma_kernel
instances, both linear_bf16in_kernel instances and both linear_generic_kernel instances."""
import ctypes

import lin_bf16in_instances as bi
import lin_instances as li
from quantize_amd import capi

ALIGNED = 1 << 20        # a 16-byte aligned stand-in address: the queries look at alignment only


def _q():
    return capi.QeQParam(ALIGNED, 8, 1, ALIGNED, ALIGNED, 1)


def test_rows_name_their_planned_kernel():
    for B, K, O, env, form, note in li.ROWS:
        with capi.knobs(**(env or {})):
            got = capi.linear_form(_q(), _q(), B, K, O)
        assert got == form, "%s (%s, env %s): the planner picks %s, the row says %s" % (
            (B, K, O), note, env, capi.LINEAR_FORMS[got], capi.LINEAR_FORMS[form])


def test_float_input_rows_name_their_kernel():
    L = capi.lib()
    for B, K, O, env, form, note in li.F_ROWS:
        with capi.knobs(**(env or {})):
            got = int(L.qe_quantlinear_float_input_path(ALIGNED, ctypes.byref(_q()), B, K, O))
        assert got == form, ((B, K, O), note, env, got)


def test_rows_cover_every_instance():
    every = li.every_instance()
    assert len(every) == 26
    missing = every - li.covered()
    assert not missing, "no row reaches %s" % sorted(missing)
    assert li.covered() <= every
    print("linear instances reached: %d of %d" % (len(li.covered()), len(every)))


def test_rows_reach_the_edges():
    by_form = lambda f: [r for r in li.ROWS if r[4] == f]
    for f in (1, 2, 3, 4):
        rows = by_form(f)
        tm = {1: 128, 2: 128, 3: 320, 4: 160}[f]
        stage = 64 if f in (1, 2) else 128
        assert any(B == 1 for B, *_ in rows), f
        assert any(1 < B < tm for B, *_ in rows), f
        assert any(B > tm and B % tm != 0 for B, *_ in rows), f
        assert any(K == stage for _, K, *_ in rows), f
        assert any(K >= 3072 for _, K, *_ in rows), f
        if f in (1, 2):
            assert any(O % 16 != 0 for _, _, O, *_ in rows) and any(O < 64 for _, _, O, *_ in rows), f
    assert {3072, 4096, 5120} <= {K for _, K, *_ in li.ROWS}
    # the two layers a 64-image ViT-B/16 batch runs on the big tiles, placed by the planner
    assert (12608, 768, 3072, None, 4) in [r[:5] for r in li.ROWS]
    assert (12608, 3072, 768, None, 3) in [r[:5] for r in li.ROWS]
    # every MFMA form sees each activation quantiser (signed / unsigned codes, per-row / per-tensor, asymmetric)
    for f in (1, 2, 3, 4):
        assert {li.XQ[i % 3] for i, r in enumerate(li.ROWS) if r[4] == f} == set(li.XQ), f


def test_query_follows_the_knobs():
    q = _q()
    with capi.knobs(QE_LIN_NJ="2", QE_LIN8="1"):
        assert capi.linear_form(q, q, 12608, 3072, 768) == 1        # QE_LIN_NJ rules out the big tiles
    with capi.knobs(QE_LIN8="0"):
        assert capi.linear_form(q, q, 12608, 3072, 768) == 2
    assert capi.linear_form(q, q, 12608, 3072, 768, dst_aligned=False) == 2   # big tiles store whole 16-byte pieces
    assert capi.linear_form(q, q, 12608, 3000, 768) == 0                       # K % 64 != 0
    bits4 = capi.QeQParam(ALIGNED, 4, 1, ALIGNED, ALIGNED, 1)
    assert capi.linear_form(bits4, q, 64, 256, 256) == 0


def test_queries_answer_from_one_plan():
    """The path and workspace queries of the fused forms agree with qe_quantlinear_form / _float_input_path on every row:
    path 1 exactly when the row runs an MFMA kernel (and needs no workspace), two passes through B*O floats otherwise; the
    bf16 form needs O % 8 == 0 and an aligned `out` as well, and the bf16-input form's workspace on path 0 is the widened
    rows in front of the float-input residual plan's own."""
    L = capi.lib()
    q = _q()
    rq = lambda bits, n_param: capi.QeRequant(ALIGNED, ALIGNED, n_param, -128.0, 127.0, bits, 1)
    rq_path = lambda B, K, O, r, codes=ALIGNED: int(L.qe_quantlinear_requant_path(q, q, B, K, O, r, codes))
    for B, K, O, env, form, note in li.ROWS:
        row = ((B, K, O), note, env)
        with capi.knobs(**(env or {})):
            fused = int(form != 0)
            assert capi.linear_path(q, q, B, K, O) == fused, row
            assert rq_path(B, K, O, rq(8, 1)) == fused, row
            assert capi.linear_residual_path(q, q, B, K, O) == fused, row
            ws = 0 if fused else B * O * 4
            assert int(L.qe_quantlinear_requant_workspace_bytes(q, q, B, K, O, rq(8, 1), ALIGNED)) == ws, row
            assert int(L.qe_quantlinear_residual_workspace_bytes(q, q, B, K, O)) == ws, row
            # what the fused epilogue cannot store: per-channel or sub-8-bit codes, codes off a 16-byte boundary
            assert rq_path(B, K, O, rq(8, O)) == (fused if O == 1 else 0), row
            assert rq_path(B, K, O, rq(4, 1)) == 0, row
            assert rq_path(B, K, O, rq(8, 1), ALIGNED + 4) == 0, row
            assert int(L.qe_quantlinear_requant_workspace_bytes(q, q, B, K, O, rq(4, 1), ALIGNED)) == B * O * 4, row
            # bf16 rows: fused exactly on an MFMA form with O % 8 == 0 and an aligned `out` (NULL reads as aligned)
            for out in (None, ALIGNED, ALIGNED + 2, ALIGNED + 8):
                want = int(form != 0 and O % 8 == 0 and (out or 0) % 16 == 0)
                assert int(L.qe_quantlinear_bf16_path(q, q, B, K, O, out)) == want, (row, out)
                assert int(L.qe_quantlinear_bf16_workspace_bytes(q, q, B, K, O, out)) == (0 if want else B * O * 4), (row, out)
        with capi.knobs(**dict(env or {}, QE_LIN_EPI="0")):
            assert rq_path(B, K, O, rq(8, 1)) == 0 and capi.linear_residual_path(q, q, B, K, O) == 0, row
            assert int(L.qe_quantlinear_residual_workspace_bytes(q, q, B, K, O)) == B * O * 4, row
            assert int(L.qe_quantlinear_bf16_path(q, q, B, K, O, ALIGNED)) == 0, row
            assert int(L.qe_quantlinear_bf16_workspace_bytes(q, q, B, K, O, ALIGNED)) == B * O * 4, row
    for B, K, O, env, form, note in li.F_ROWS:
        row = ((B, K, O), note, env)
        with capi.knobs(**(env or {})):
            assert int(L.qe_quantlinear_float_input_residual_path(ALIGNED, q, B, K, O)) == form, row
            ws = int(L.qe_quantlinear_float_input_residual_workspace_bytes(ALIGNED, q, B, K, O))
            assert ws == (0 if form else B * O * 4), row
            # bf16 activations: linear_bf16in_kernel where linear_f32_mfma_kernel would run and x is 16-byte aligned, with
            # no workspace; else the widened rows (B*K floats, rounded up to 16 bytes) in front of the float-input residual
            # plan's own workspace
            for x in (ALIGNED, ALIGNED + 2):
                path = int(form == 1 and x % 16 == 0)
                assert int(L.qe_quantlinear_bf16_input_path(x, q, B, K, O)) == path, (row, x)
                want = 0 if path else (B * K * 4 + 15) // 16 * 16 + ws
                assert int(L.qe_quantlinear_bf16_input_workspace_bytes(x, q, B, K, O)) == want, (row, x)
        with capi.knobs(**dict(env or {}, QE_LIN_EPI="0")):
            assert int(L.qe_quantlinear_float_input_residual_path(ALIGNED, q, B, K, O)) == 0, row
            # the widened form follows the float-input plan under the knob
            ws0 = int(L.qe_quantlinear_float_input_residual_workspace_bytes(ALIGNED, q, B, K, O))
            assert ws0 == B * O * 4, row
            assert int(L.qe_quantlinear_bf16_input_workspace_bytes(ALIGNED + 2, q, B, K, O)) == (B * K * 4 + 15) // 16 * 16 + ws0, row
    for B, K, O, w_bits, off, path, note in bi.ROWS:
        w = capi.QeQParam(ALIGNED, w_bits, 1, ALIGNED, ALIGNED, 1)
        assert int(L.qe_quantlinear_bf16_input_path(ALIGNED + off, w, B, K, O)) == path, note
        ws = int(L.qe_quantlinear_float_input_residual_workspace_bytes(ALIGNED, w, B, K, O))
        want = 0 if path else (B * K * 4 + 15) // 16 * 16 + ws
        assert int(L.qe_quantlinear_bf16_input_workspace_bytes(ALIGNED + off, w, B, K, O)) == want, note
