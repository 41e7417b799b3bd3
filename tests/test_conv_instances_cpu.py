"""CPU: the conv instance table (tests/conv_instances.py) against the host-side plan (qe_quantconv2d_plan_info,
qe_conv_mfma_has_instance: no device work).  Every row names the instance the planner picks for it; together the rows reach
every instance a request can select; every compiled instance is either reached or listed as unreachable with its reason; and
no plan of the sweep grid names an instance the library does not compile."""
import ctypes
import time

import conv_instances as ci
from quantize_amd import capi

A = ci.ALIGNED


def _lib_queries(shape, xb, wb):
    sh = capi.conv_shape(*shape[:5], shape[5], shape[5], shape[6], shape[7])
    return sh, ci.qparam(xb), ci.qparam(wb)


def test_rows_name_their_planned_instance():
    for shape, xb, wb, env, expected, note in ci.ROWS:
        with capi.knobs(**(env or {})):
            info = ci.plan(shape, xb, wb)
        got = ci.launched(info)
        assert expected in got, "%s A%dW%d env %s (%s): the planner picks %s, the row says %s" % (
            shape, xb, wb, env, note, sorted(got, key=str), expected)
        assert expected[0] == "pre" or not expected[-1] or expected[0] in ci.FLAT, expected     # the fp32 instance
    assert len({(r[0], r[1], r[2], str(r[3])) for r in ci.ROWS}) == len(ci.ROWS), "duplicate rows"


def test_instance_counts():
    """What the selectors compile, by family (the figures of DESIGN.md)."""
    every = ci.every_instance()
    count = lambda f: sum(1 for i in every if i[0] == f)
    assert {f: count(f) for f in ("halo", "stem", "ws", "sm2", "flat", "flat_s2", "flat_x4", "flatg", "flatd", "pre")} == {
        "halo": 81, "stem": 8, "ws": 18, "sm2": 18, "flat": 30, "flat_s2": 2, "flat_x4": 9, "flatg": 4, "flatd": 4, "pre": 10}
    # one PATCH form on the halo kernel, two on the stem, one per re-quantising two-strip instance
    assert sum(1 for i in every if i[0] in ("halo", "stem", "sm2") and i[-1]) == 1 + 2 + 6
    assert ("halo", 0, 7, 9, 1, True, True) in every


def test_rows_cover_every_reachable_instance():
    t0 = time.time()
    reached, n_plans, _ = ci.scan()
    print("sweep: %d plans in %.1f s, %d instances reached" % (n_plans, time.time() - t0, len(reached)))
    assert n_plans > 100000
    covered = ci.covered()
    assert not reached - covered, "no row reaches %s" % sorted(reached - covered, key=str)
    assert not covered - reached, "rows reach what the sweep does not: %s" % sorted(covered - reached, key=str)
    for fam in ("halo", "ws", "sm2", "stem", "flat", "flat_s2", "flat_x4", "flatg", "flatd", "pre"):
        print("%-8s compiled %3d reachable %3d covered %3d" % (fam, sum(i[0] == fam for i in ci.every_instance()),
                                                              sum(i[0] == fam for i in reached), sum(i[0] == fam for i in covered)))


def test_unreachable_list_is_exact():
    """A planner change that makes a listed instance reachable, or a new instantiation in a selector, fails here until a row
    or a reason is added."""
    every, reached = ci.every_instance(), ci.reachable()
    assert reached <= every, "the planner selects what no selector compiles: %s" % sorted(reached - every, key=str)
    assert every - reached == set(ci.UNREACHABLE), (sorted(every - reached - set(ci.UNREACHABLE), key=str),
                                                    sorted(set(ci.UNREACHABLE) - (every - reached), key=str))
    assert all(isinstance(why, str) and why for why in ci.UNREACHABLE.values())


def test_every_plan_of_the_grid_can_launch():
    """launch_conv_mfma's "never for a plan of plan_conv": every MFMA-route plan names a compiled instance, fits its LDS
    limit, has a grid, and takes the PATCH form only under plan_rq_patch's conditions."""
    problems = ci.scan()[2]
    assert not problems, "%d plans, first: %s" % (len(problems), problems[:5])


def test_has_instance_rejects_what_no_selector_compiles():
    has = capi.conv_mfma_has_instance
    assert has(1, 0, 7, 9, 1, 1, 0, 1, 1) and not has(1, 0, 4, 9, 1, 1, 0, 1, 1)      # the one halo PATCH form
    assert not has(1, 0, 7, 9, 2, 1, 0, 0, 0) and not has(1, 0, 3, 1, 1, 1, 0, 0, 0)  # NS > 1 is 1x1 only; no NIW 3
    assert not has(1, 2, 4, 1, 1, 1, 0, 0, 0) and not has(1, 3, 2, 1, 1, 1, 0, 0, 0)  # 1x4 waves: NIW 2 | 1; no cfg 3
    assert not has(2, 0, 7, 9, 1, 3, 0, 0, 0) and not has(2, 1, 7, 9, 1, 1, 0, 0, 0)  # ws: split 1 | 2 | 4, 4x1 waves only
    assert not has(4, 1, 4, 0, 1, 1, 0, 0, 0) and not has(4, 2, 2, 0, 1, 1, 0, 1, 1)  # stem: NIW 7 at 2x2; PATCH at NIW 7 only
    assert not has(5, 0, 7, 1, 3, 1, 1, 0, 0) and not has(5, 1, 7, 1, 1, 1, 1, 0, 0)  # flat: NS 1 | 2 | 4; 2x2 waves: NIW 4
    assert not has(6, 0, 7, 1, 4, 1, 1, 0, 0) and not has(7, 0, 7, 1, 2, 1, 1, 0, 0)  # flat s2: NS 2; x4: prepared tables only
    assert not has(0, 0, 7, 1, 1, 1, 0, 0, 0) and not has(9, 0, 7, 1, 1, 1, 0, 0, 0) and not has(1, 0, 7, 2, 1, 1, 0, 0, 0)


def test_the_queries_answer_from_one_plan():
    """conv_path, requant_path and the workspace queries agree with plan_info on every row and named shape, in every bit
    pair, under the row's knobs."""
    L = capi.lib()
    rq = ci.requant8()
    cases = [(r[0], r[3]) for r in ci.ROWS] + [(s, None) for s in ci._named_shapes()]
    for shape, env in cases:
        with capi.knobs(**(env or {})):
            for xb, wb in ci.BITS:
                sh, x, w = _lib_queries(shape, xb, wb)
                what = (shape, xb, wb, env)
                info = capi.conv_plan_info(sh, x, w)
                assert capi.conv_path(sh, x, w) == int(capi.CONV_ROUTES[info.route] != "generic"), what
                assert capi.workspace_bytes(sh, xb, wb) == info.total, what
                assert int(L.qe_quantconv2d_prepared_workspace_bytes(ctypes.byref(sh), xb, wb)) == info.total - info.prep_total, what
                assert int(L.qe_conv_prepared_bytes(ctypes.byref(sh), xb, wb)) == info.prep_total or shape[0] * shape[1] * shape[2] * shape[3] < 64, what
                ri = capi.conv_plan_info(sh, x, w, rq)
                assert capi.requant_path(sh, x, w, rq) == ri.fused, what
                scratch = (ri.total - ri.prep_total + 255) // 256 * 256
                need = int(L.qe_quantconv2d_requant_workspace_bytes(ctypes.byref(sh), ctypes.byref(x), ctypes.byref(w), ctypes.byref(rq)))
                assert need == (scratch if ri.fused else scratch + ri.y_bytes), what
                assert ri.rq == int(ri.fused and capi.CONV_ROUTES[ri.route] == "mfma") and (ri.patch <= ri.rq), what
                assert info.rq == 0 and info.patch == 0 and info.fused == 0, what


def test_plan_info_checks_its_arguments():
    L = capi.lib()
    sh, x, w = _lib_queries((1, 8, 8, 8, 8, 3, 1, 1), 8, 8)
    info = capi.QeConvPlanInfo()
    assert L.qe_quantconv2d_plan_info(None, x, w, None, None, None, info) == 4
    assert L.qe_quantconv2d_plan_info(sh, None, w, None, None, None, info) == 4
    assert L.qe_quantconv2d_plan_info(sh, x, w, None, None, None, None) == 4
    bad = capi.conv_shape(1, 8, 8, 8, 8, 3, 3, 0, 1)
    assert L.qe_quantconv2d_plan_info(bad, x, w, None, None, None, info) == 4


def _row_plans(*families):
    for row in ci.rows_of(*families):
        with capi.knobs(**(row[3] or {})):
            info = ci.plan(row[0], row[1], row[2])
            yield row, info, ci.edges(row[0], row[1], row[2], info)


def test_rows_stay_small():
    """N <= 3 unless the tile's image group needs more; output planes of at most 32 x 32 unless the row is there for
    several pixel tiles of a wide tile or for a gather's wide rows; a reduction the oracle's three modes finish in about a
    second (1.5e8 multiply-adds at its measured rate) -- most rows are a hundred times smaller."""
    for (shape, xb, wb, env, expected, note), info, edges in _row_plans(*{ci.family_of(r[4]) for r in ci.ROWS}):
        N, IC, H, W, OC, K, stride, pad = shape
        assert N <= 3 or (info.gi > 1 and N <= 2 * info.gi), (shape, note)
        assert info.oh * info.ow <= 1024 or expected[0] == "pre" or edges & {"several pixel tiles", "several row tiles"}, (shape, note)
        assert H * W <= 112 * 56 and N * OC * info.oh * info.ow * IC * K * K <= 1.5e8, (shape, note)


def test_rows_reach_the_edges():
    """Across each family's rows: what its kernels branch on (conv_instances.edges reads it off the plan)."""
    def reached(*families):
        out = set()
        for _, _, e in _row_plans(*families):
            out |= e
        return out

    common = {"ragged OC tile", "several OC tiles", "several stages", "several image groups", "IC % 32 != 0",
              "IC % 16 != 0", "sub-8-bit weights"}
    lane_pixel = common | {"partial row tile", "several row tiles", "partial image group", "class table",
                           "no class table: bands overlap", "stride 2"}
    want = {
        "halo": lane_pixel | {"OC below one strip", "NCH padded to NS", "ROWMUL / COLMUL", "no class table: too many classes"},
        "ws": lane_pixel, "sm2": lane_pixel,
        "stem": {"ragged OC tile", "several OC tiles", "OC below one strip", "partial row tile", "several row tiles",
                 "class table", "stride 2"},
        "flat": common | {"OC below one strip", "partial pixel tile", "several pixel tiles", "NCH padded to NS"},
        "flat_s2": {"ragged OC tile", "several OC tiles", "several stages", "several pixel tiles", "IC % 32 != 0"},
        "flat_x4": common | {"partial pixel tile", "several pixel tiles", "NCH padded to NS"},
        "flatg": common | {"49-pixel planes", "56-pixel planes", "partial image group", "NCH padded to NS"},
    }
    for fam, edges in want.items():
        got = reached(fam)
        assert edges <= got, "%s rows never reach: %s" % (fam, sorted(edges - got))
    # every split of the staging threads on both kernels that have one, every subsample2 width
    assert {r[4][2] for r in ci.rows_of("ws")} == {1, 2, 4} and {r[4][2] for r in ci.rows_of("sm2")} == {1, 2, 4}
    assert {r[4][2] for r in ci.ROWS if r[4][:2] == ("pre", "sub2")} == {3, 4, 5, 6, 7, 8}
    # the gathers' last piece of a row: 4 + 2 + 1 bytes on subsample2, ragged on the others
    ow = lambda kind: {info.ow for row, info, _ in _row_plans(kind)}
    assert any(v % 8 == 7 for v in ow("sub2")) and any(v % 8 for v in ow("sub_x4")) and any(v % 8 for v in ow("sub_wide"))
    assert {v % 4 for v in ow("sub_narrow")} >= {1, 2, 3}
    assert {r[1] for r in ci.rows_of("expand")} >= {4, 3}


def test_the_queries_follow_the_knobs():
    """One row per knob: the plan names another instance under the knob and the old one again afterwards."""
    flips = [
        ((2, 128, 14, 14, 130, 3, 1, 1), 8, 8, {"QE_SM2": "0", "QE_WS": "0"}), ((5, 64, 7, 7, 130, 3, 1, 1), 8, 8, {"QE_WS": "0"}),
        ((2, 256, 28, 28, 160, 1, 1, 0), 8, 8, {"QE_FLAT_NIW": "4"}), ((2, 256, 28, 28, 160, 1, 1, 0), 8, 8, {"QE_FLAT_NS": "1"}),
        ((3, 256, 14, 14, 140, 1, 2, 0), 8, 8, {"QE_SUBSAMPLE": "0"}), ((3, 256, 14, 14, 140, 1, 2, 0), 8, 8, {"QE_SUB2": "0"}),
        ((2, 128, 56, 56, 160, 1, 2, 0), 8, 8, {"QE_FLAT_S2": "0"}), ((5, 160, 7, 7, 200, 1, 1, 0), 8, 8, {"QE_FLATG": "0"}),
        ((2, 96, 28, 28, 130, 1, 1, 0), 4, 8, {"QE_X4": "0"}), ((2, 64, 28, 28, 130, 1, 2, 0), 4, 8, {"QE_SUB_X4": "0"}),
        ((4, 2048, 7, 7, 512, 1, 1, 0), 8, 8, {"QE_FLATD": "0"}), ((4, 2048, 7, 7, 512, 1, 1, 0), 8, 8, {"QE_FLATD8": "1"}),
        ((2, 64, 28, 28, 256, 1, 1, 0), 8, 8, {"QE_PWR": "0"}),
    ]
    for shape, xb, wb, env in flips:
        key = lambda i: (i.route, i.family, i.niw, i.ns, i.pre, i.fd_w8, i.expand, i.sub_x4)
        before = key(ci.plan(shape, xb, wb))
        with capi.knobs(**env):
            assert key(ci.plan(shape, xb, wb)) != before, (shape, env)
        assert key(ci.plan(shape, xb, wb)) == before, (shape, env)
    # the epilogue knobs: the PATCH form, the class table
    shape = (1, 64, 16, 16, 64, 3, 1, 1)
    assert ci.plan(shape, rq=True).patch == 1 and ci.plan(shape, rq=True, codes=A + 1).patch == 0
    with capi.knobs(QE_RQ_PATCH="0"):
        assert ci.plan(shape, rq=True).patch == 0 and ci.plan(shape, rq=True).rq == 1
    assert ci.plan(shape).ctab == 1
    with capi.knobs(QE_CTAB="0"):
        assert ci.plan(shape).ctab == 0
    assert ci.plan(shape, rq=True).patch == 1 and ci.plan(shape).ctab == 1
