"""CPU: the float-input conv instance table (tests/f32_instances.py) names the kernel the planner picks for each row
(qe_conv_f32_plan_info: a host-only query), every edge a row claims is recomputed from the plan, the rows reach all 11
instances launch_conv_f32 can select and every edge of EDGES, the path and workspace queries answer from the same plan, and
over a sweep of 6e5 shapes every plan the query calls ok keeps what conv_f32_mfma_kernel / conv_f32_stem_kernel assume
about it (staging threads, LDS, pixel slots, padded groups, grid, 32-bit offsets)."""
import collections
import ctypes
import itertools

import f32_instances as fi
from quantize_amd import capi

ALIGNED = 1 << 20        # a 16-byte aligned stand-in address: the queries look at no operand


def _q(bits=8):
    return capi.QeQParam(ALIGNED, bits, 1, ALIGNED, ALIGNED, 1)


def _plan(shape):
    return capi.conv_f32_plan_info(capi.conv_shape(*shape))


def _cdiv(a, b):
    """C's integer division (towards zero), as the planner and every kernel of the library compute the output plane: a
    window larger than the padded image still gives one output row where the stride exceeds the deficit."""
    return a // b if a >= 0 else -(-a // b)


def _name(p):
    return capi.F32_KERNELS[p.kernel] if p.ok else None


def test_rows_name_their_planned_instance_and_edges():
    assert len(capi.F32_KERNELS) == 11 and set(capi.F32_KERNELS) == fi.every_instance()
    for r in fi.ROWS:
        p = _plan(fi.shape_of(r))
        assert _name(p) == r.instance, "%s: the planner picks %s" % (fi.row_id(r), _name(p))
        assert bool(p.stem) == (r.instance in fi.STEMS)
        for e in r.note.split():
            assert e in fi.EDGES, (fi.row_id(r), e)
            assert fi.EDGES[e](r, p), "%s claims %s, its plan does not have it" % (fi.row_id(r), e)
        assert fi.macs(r) <= 21e6, (fi.row_id(r), fi.macs(r))
    assert len({fi.shape_of(r) for r in fi.ROWS}) == len(fi.ROWS)


def test_rows_cover_every_instance_and_edge():
    every = fi.every_instance()
    assert len(every) == 11
    assert fi.covered() == every, "no row reaches %s" % sorted(every - fi.covered())
    missing = set(fi.EDGES) - fi.claimed()
    assert not missing, "no row claims %s" % sorted(missing)
    for inst in every:
        # pass B of the GPU test (three non-zero splits, bit-exact) needs a row with IC * KH * KW <= 64 on every instance
        assert any(r.IC * r.KH * r.KW <= 64 for r in fi.rows_of(inst)), inst
    for inst in fi.MAINS:
        rows = fi.rows_of(inst)
        assert len(rows) >= 4, inst
        assert any(fi.weights_of(r)[4] != "zero" for r in rows), inst          # the S_x correction runs
        assert any("oc_ragged" in r.note.split() for r in rows), inst
        assert any("gi" in r.note.split() for r in rows), inst
    print("float-input conv instances reached: %d of %d, %d rows, %d edges" % (len(fi.covered()), len(every), len(fi.ROWS),
                                                                              len(fi.EDGES)))


def test_block_map_reaches_every_tile_once():
    """The kernels' own decode of blockIdx.x (tile_grid's device half), over the whole grid of every row."""
    for r in fi.ROWS:
        p = _plan(fi.shape_of(r))
        seen = collections.Counter()
        for bid in range(p.blocks):
            idx = bid >> 3
            j, ot = divmod(idx, p.n_oc_tiles)
            c = j // p.chunk
            pt = (c * 8 + (bid & 7)) * p.chunk + (j - c * p.chunk)
            if pt < p.n_pix_tiles:
                seen[(pt, ot)] += 1
        assert len(seen) == p.n_pix_tiles * p.n_oc_tiles and set(seen.values()) == {1}, fi.row_id(r)
        assert p.n_pix_tiles == -(-r.N // p.GI) * p.tiles_h and p.tiles_h == -(-p.OH // p.TH), fi.row_id(r)
        assert p.n_oc_tiles * fi.mt(r.instance) == p.OCP >= r.OC > p.OCP - fi.mt(r.instance), fi.row_id(r)


def test_path_and_workspace_queries_answer_from_the_plan():
    L = capi.lib()
    cases = [(fi.shape_of(r), None, r.instance) for r in fi.ROWS] + [(f[:9], f[9], f[10]) for f in fi.FALLBACK]
    for shape, env, inst in cases:
        sh = capi.conv_shape(*shape)
        with capi.knobs(**(env or {})):
            p = capi.conv_f32_plan_info(sh)
            assert _name(p) == inst, (shape, env, _name(p))
            assert capi.float_input_path(sh, _q()) == p.ok == int(inst is not None), (shape, env)
            for bits in (8, 3):
                ws = int(L.qe_quantconv2d_float_input_workspace_bytes(ctypes.byref(sh), bits))
                assert ws == p.total and (ws > 0) == bool(p.ok), (shape, env, ws, p.total)
            if p.ok:
                mtile = fi.mt(inst)
                wt = (shape[5] * 2 if p.stem else p.KK * p.NG) * p.OCP * 16 * 2
                assert p.ep_off == -(-wt // 256) * 256 and p.total == -(-(p.ep_off + 3 * p.OCP * 4) // 256) * 256, shape
                assert p.OCP % mtile == 0
    # the query checks its arguments like the other entry points
    assert L.qe_conv_f32_plan_info(None, ctypes.byref(capi.QeConvF32Plan())) == 4
    assert L.qe_conv_f32_plan_info(ctypes.byref(capi.conv_shape(1, 8, 8, 8, 8, 3, 3, 0, 1)), ctypes.byref(capi.QeConvF32Plan())) == 4
    assert L.qe_conv_f32_plan_info(ctypes.byref(capi.conv_shape(1, 8, 8, 8, 8, 3, 3, 1, 1)), None) == 4


# ---- the sweep ---------------------------------------------------------------------------------------------------------
GRID = dict(N=(1, 3, 9, 130), IC=(1, 3, 4, 5, 8, 17, 64, 80), H=(1, 4, 7, 15, 57, 230), W=(3, 4, 5, 7, 16, 57, 225, 449),
            OC=(8, 65, 130), K=((1, 1), (3, 3), (1, 3), (3, 1), (7, 1), (1, 7), (2, 2), (5, 5), (8, 8), (9, 9)),
            stride=(1, 2, 3, 7), pad=(0, 1, 3))
# tiny output planes of huge images (a stride as large as the image), many images, wide output-channel counts: where a tile
# takes up to 128 images and the kernels' 32-bit offsets are at stake
HUGE = dict(N=(1, 8, 9, 16, 128, 200), IC=(8, 15, 16, 31), H=(1 << 20, 1 << 22, (1 << 24) - 1, 1 << 24), W=(4, 5, 8, 16),
            OC=(8, 65, 1 << 24, 1 << 25), K=((1, 1), (1, 3), (3, 1)), stride=(1, 0, -1), pad=(0, 1))


def _sweep():
    for g in (GRID, HUGE):
        for N, IC, H, W, OC, (KH, KW), s, pad in itertools.product(*(g[k] for k in ("N", "IC", "H", "W", "OC", "K", "stride", "pad"))):
            if s <= 0:
                s = H if s == 0 else H // 2        # HUGE: one or two output rows
            yield N, IC, H, W, OC, KH, KW, s, pad


def test_sweep_plans_keep_what_the_kernels_assume():
    f = capi.lib().qe_conv_f32_plan_info
    sh, p = capi.QeConvShape(), capi.QeConvF32Plan()
    psh, pp = ctypes.byref(sh), ctypes.byref(p)
    names = capi.F32_KERNELS
    n = n_ok = 0
    reach = collections.defaultdict(set)          # instance -> {"gi_ragged", "row_ragged"} the planner can produce
    per_instance = collections.Counter()
    for shape in _sweep():
        N, IC, H, W, OC, KH, KW, s, pad = shape
        sh.N, sh.IC, sh.H, sh.W, sh.OC, sh.KH, sh.KW, sh.stride, sh.padding = shape
        assert f(psh, pp) == 0
        n += 1
        if not p.ok:
            continue
        n_ok += 1
        inst = names[p.kernel]
        per_instance[inst] += 1
        WM, WN, NIW = fi.WAVES[inst]
        NQ = (W + 3) // 4
        assert p.OH == _cdiv(H + 2 * pad - KH, s) + 1 and p.OW == _cdiv(W + 2 * pad - KW, s) + 1 and p.KK == KH * KW <= 64, shape
        assert W >= 4 and 1 <= p.TH <= p.OH and p.GI >= 1, shape
        assert p.OCP % (32 * WM) == 0 and p.OCP - 32 * WM < OC <= p.OCP and p.n_oc_tiles * 32 * WM == p.OCP, shape
        gsz = p.GI * p.IHT * p.IWP
        if p.stem:
            assert inst in fi.STEMS and IC <= 4 and KH <= 8 and KW <= 8 and p.GI == 1 and p.NG == 1, shape
            assert p.TH * p.OW <= 32 * NIW * WN, shape
            assert p.IHT == (p.TH - 1) * s + KH and p.IWP == (p.OW - 1) * s + 8, shape       # the fragment reads 8 columns
            assert p.lds == (3 * gsz + 64) * 8 + gsz * 4, shape
            assert (inst == "Stem4x1x7") == (OC > 64), shape
            if inst == "Stem2x2x4":
                assert p.TH * p.OW <= 256, shape
            assert IC * H * W < 1 << 31 and OC * p.OH * p.OW < 1 << 32, shape
        else:
            NS = fi.ns(inst)
            assert inst in fi.MAINS and IC >= 8, shape
            assert 2 * NS * p.GI * p.IHT * NQ <= 256, shape                  # one staging thread per (group, k-half, unit)
            assert p.GI * p.TH * p.OW <= 32 * NIW * WN, shape
            assert p.NG % NS == 0 and 16 * p.NG >= IC > 16 * (p.NG - NS), shape
            assert p.ROWMUL == (s if KH == 1 else 1) and p.COLMUL == (s if KW == 1 else 1), shape
            assert p.IHT == (p.TH if KH == 1 and s > 1 else (p.TH - 1) * s + KH), shape
            assert p.IWP == (p.OW if KW == 1 and s > 1 else (p.OW - 1) * s + KW), shape
            assert p.lds == (6 * NS * gsz + 64) * 16 + 2 * NS * gsz * 4, shape
            assert p.GI == 1 or p.TH == p.OH, shape                           # several images per tile: whole images
            # 32-bit offsets: u_off = gi IC H W + ... (int) and voff = (gi OC + oc) OH OW + pixel (uint32_t), gi < GI
            assert p.GI * IC * H * W < 1 << 31, shape
            assert p.GI * OC * p.OH * p.OW < 1 << 32, shape
            if p.GI > 1 and N % p.GI:
                reach[inst].add("gi_ragged")
            if p.OH % p.TH:
                reach[inst].add("row_ragged")
        assert p.lds <= 65536, shape
        assert p.tiles_h == -(-p.OH // p.TH) and p.n_pix_tiles == -(-N // p.GI) * p.tiles_h, shape
        # the grid holds the last (pixel tile, oc tile) of the kernels' block decode
        c_max = (p.n_pix_tiles - 1) // p.chunk // 8
        r_max = p.chunk - 1 if c_max * 8 * p.chunk + p.chunk - 1 <= p.n_pix_tiles - 1 else (p.n_pix_tiles - 1) % p.chunk
        assert p.chunk >= 1 and (c_max * p.chunk + r_max + 1) * p.n_oc_tiles * 8 <= p.blocks < 1 << 31, shape
        assert p.total < 1 << 31 and p.ep_off + 3 * p.OCP * 4 <= p.total, shape
    print("sweep: %d shapes, %d on an MFMA kernel: %s" % (n, n_ok, dict(per_instance)))
    assert n > 500000 and set(per_instance) == fi.every_instance()
    # the table has a ragged image group and a ragged row tile on every main instance that can have one
    for inst in fi.MAINS:
        for e in sorted(reach[inst]):
            assert any(e in r.note.split() for r in fi.rows_of(inst)), "%s can have %s (sweep), no row claims it" % (inst, e)
        for e in ("gi_ragged", "row_ragged"):
            if e not in reach[inst]:
                assert not any(e in r.note.split() for r in fi.rows_of(inst))
                print("%s: no plan of the sweep has %s" % (inst, e))


def test_offset_guard_reads_the_chosen_gi():
    """u_off = gi IC H W + ... is formed in int and voff = (gi OC + oc) OH OW + pixel in uint32_t, with gi < GI.  The planner's
    first guard (IC H W 8 < 2^31) was written for tiles of up to 8 images, but a 1 x 1 output plane takes up to 128: the
    second guard reads the GI the planner chose and leaves such a shape to the VALU kernel.  GI itself is not capped."""
    IC, H, W = 15, 1 << 22, 4                        # 2.5e8 elements per image: passes the first guard
    assert IC * H * W * 8 < 1 << 31
    p = _plan((8, IC, H, W, 8, 1, 1, H, 0))
    assert p.ok and p.GI == 8 and p.OH == p.OW == 1
    for N in (9, 16, 128, 200):
        assert N * IC * H * W >= 1 << 31 and not _plan((N, IC, H, W, 8, 1, 1, H, 0)).ok, N
    # ... and the outputs of a tile: GI OC OH OW < 2^32
    OC = 1 << 25
    p = _plan((127, 8, 4, 4, OC, 1, 1, 4, 0))
    assert p.ok and p.GI == 127 and 127 * OC < 1 << 32
    assert not _plan((128, 8, 4, 4, OC, 1, 1, 4, 0)).ok
    # tiny images still share a tile far beyond 8 of them
    p = _plan((200, 16, 4, 4, 8, 1, 1, 4, 0))
    assert p.ok and p.GI == 128
