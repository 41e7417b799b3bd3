"""One table for the float-input convolution kernels (qe_conv_f32.hip), shared by the CPU coverage test and the GPU tests.

ROWS: (N, IC, H, W, OC, KH, KW, stride, pad, instance, note).  `instance` is the F32Kernel that qe_conv_f32_plan_info must name
for the shape (capi.F32_KERNELS): conv_f32_stem_kernel<4,1,7 | 2,2,4 | 2,2,7> and conv_f32_mfma_kernel<4,1,4|7,1|2> /
<2,2,2|4,1|2>.  `note` is a space-separated list of the edges (keys of EDGES) the row is there for;
tests/test_f32_instances_cpu.py recomputes each of them from the plan.  The weight edges also say which weights the GPU tests
draw for the row (weights_of): sN / uN signed / unsigned N-bit codes (default s8), per_tensor (default: per channel),
nobias, zw0 (all zero points 0) and zw_tile_mix (zero points 0 on the first output-channel tile only).

FALLBACK: (N, IC, H, W, OC, KH, KW, stride, pad, env, instance or None, note): both sides of each planner boundary; None is
the order-preserving VALU kernel (qe_conv_generic.hip), whose contract is bit-identity with the reference's fmaf chain.

Every row stays below about 20 M multiply-adds, so that the C oracle answers in a fraction of a second."""
import collections

Row = collections.namedtuple("Row", "N IC H W OC KH KW stride pad instance note")

STEMS = ("Stem4x1x7", "Stem2x2x4", "Stem2x2x7")
MAINS = ("M4x1x4", "M4x1x4S2", "M4x1x7", "M4x1x7S2", "M2x2x2", "M2x2x2S2", "M2x2x4", "M2x2x4S2")
# <WM, WN, NIW> of an instance: MT = 32 WM output channels, 32 NIW WN pixel slots
WAVES = {"Stem4x1x7": (4, 1, 7), "Stem2x2x4": (2, 2, 4), "Stem2x2x7": (2, 2, 7),
         "M4x1x4": (4, 1, 4), "M4x1x4S2": (4, 1, 4), "M4x1x7": (4, 1, 7), "M4x1x7S2": (4, 1, 7),
         "M2x2x2": (2, 2, 2), "M2x2x2S2": (2, 2, 2), "M2x2x4": (2, 2, 4), "M2x2x4S2": (2, 2, 4)}
PATCH_BYTES = 4 * 32 * 36 * 4      # the four waves' store patches, which overwrite the dead halo image


def mt(inst):
    return 32 * WAVES[inst][0]


def slots(inst):
    """Pixel slots of a tile: 32 x NIW x WN."""
    return 32 * WAVES[inst][2] * WAVES[inst][1]


def ns(inst):
    return 2 if inst.endswith("S2") else 1


def image_bytes(r, p):
    """LDS bytes of the halo image (what the store patches may overwrite)."""
    return 3 * p.IHT * p.IWP * 8 if p.stem else 6 * ns(r.instance) * p.GI * p.IHT * p.IWP * 16


def _patch_shape(r, p):
    """Everything the 16-byte patch stores need except the size of the halo image: one image per tile, 16-byte aligned
    planes (the first row tile of an image then starts aligned) and a whole 32 x 32 tile (full output-channel tile, 32
    valid pixels)."""
    return p.GI == 1 and (p.OH * p.OW) % 4 == 0 and r.OC >= mt(r.instance) and p.TH * p.OW >= 32


def _w(note):
    for t in note.split():
        if len(t) == 2 and t[0] in "su" and t[1].isdigit():
            return t
    return "s8"


def weights_of(r):
    """(bits, signed, per_tensor, bias, zero-point mode 'rand' | 'zero' | 'tile_mix') of a row."""
    t = r.note.split()
    w = _w(r.note)
    zmode = "zero" if "zw0" in t else ("tile_mix" if "zw_tile_mix" in t else "rand")
    return int(w[1]), w[0] == "s", "per_tensor" in t, "nobias" not in t, zmode


_is1x1s = lambda r: r.KH == 1 and r.KW == 1 and r.stride > 1
_main = lambda r: r.instance in MAINS
_stem = lambda r: r.instance in STEMS
_ni = lambda p: (p.TH * p.OW + 31) // 32

# edge -> predicate over (row, plan): what the row must really have to claim it
EDGES = {
    # tile geometry
    "gi": lambda r, p: p.GI > 1,
    "gi_ragged": lambda r, p: p.GI > 1 and r.N % p.GI != 0,
    "gi>8": lambda r, p: p.GI > 8,
    "row_ragged": lambda r, p: p.OH % p.TH != 0,
    "row_tiles": lambda r, p: p.tiles_h >= 2,
    "oc_ragged": lambda r, p: r.OC % mt(r.instance) != 0,
    "oc<32": lambda r, p: r.OC < 32,
    "oc=65": lambda r, p: r.OC == 65 and mt(r.instance) == 128,
    "oc%32": lambda r, p: r.OC % 32 != 0,
    "w%4=1": lambda r, p: r.W % 4 == 1,
    "w%4=2": lambda r, p: r.W % 4 == 2,
    "w%4=3": lambda r, p: r.W % 4 == 3,
    "w=4": lambda r, p: r.W == 4,
    "ic%16<8": lambda r, p: _main(r) and 1 <= r.IC % 16 <= 7,
    "ic%16>8": lambda r, p: _main(r) and 9 <= r.IC % 16 <= 15,
    "ic=8": lambda r, p: r.IC == 8,
    "ng_odd_s2": lambda r, p: ns(r.instance) == 2 and ((r.IC + 15) // 16) % 2 == 1 and p.NG == (r.IC + 15) // 16 + 1,
    "pix%8": lambda r, p: p.n_pix_tiles % 8 != 0,
    "pix>8": lambda r, p: p.n_pix_tiles > 8,
    "ow_limit": lambda r, p: p.OW == slots(r.instance),
    "one_tile_slot": lambda r, p: p.GI * p.TH * p.OW <= 32,
    # kernel window
    "1x1s2_pad": lambda r, p: _is1x1s(r) and r.stride == 2 and r.pad > 0,
    "1x1s2_nopad": lambda r, p: _is1x1s(r) and r.stride == 2 and r.pad == 0,
    "1x1s3_pad": lambda r, p: _is1x1s(r) and r.stride == 3 and r.pad > 0,
    "1x1s3_nopad": lambda r, p: _is1x1s(r) and r.stride == 3 and r.pad == 0,
    "1x3": lambda r, p: (r.KH, r.KW) == (1, 3),
    "3x1": lambda r, p: (r.KH, r.KW) == (3, 1),
    "1x7": lambda r, p: (r.KH, r.KW) == (1, 7),
    "7x1": lambda r, p: (r.KH, r.KW) == (7, 1),
    "rowmul!=colmul": lambda r, p: _main(r) and p.ROWMUL != p.COLMUL,
    "2x2": lambda r, p: (r.KH, r.KW) == (2, 2),
    "5x5": lambda r, p: (r.KH, r.KW) == (5, 5),
    "8x8": lambda r, p: (r.KH, r.KW) == (8, 8) and p.KK == 64,
    "stride>k": lambda r, p: r.stride > max(r.KH, r.KW) > 1,
    "pad0": lambda r, p: r.pad == 0 and r.KH * r.KW > 1,
    # store path
    "scalar_stores": lambda r, p: (p.OH * p.OW) % 4 != 0,
    "patch_stores": lambda r, p: _patch_shape(r, p) and image_bytes(r, p) >= PATCH_BYTES,
    "halo_small": lambda r, p: _patch_shape(r, p) and image_bytes(r, p) < PATCH_BYTES,
    # the stem kernel
    "stem_ic1": lambda r, p: _stem(r) and r.IC == 1,
    "stem_ic2": lambda r, p: _stem(r) and r.IC == 2,
    "stem_ic3": lambda r, p: _stem(r) and r.IC == 3,
    "stem_ic4": lambda r, p: _stem(r) and r.IC == 4,
    "stem_kw1": lambda r, p: _stem(r) and r.KW == 1,
    "stem_kw3": lambda r, p: _stem(r) and r.KW == 3,
    "stem_kw4": lambda r, p: _stem(r) and r.KW == 4,
    "stem_kw5": lambda r, p: _stem(r) and r.KW == 5,
    "stem_kw7": lambda r, p: _stem(r) and r.KW == 7,
    "stem_kw8": lambda r, p: _stem(r) and r.KW == 8,
    "stem_s1": lambda r, p: _stem(r) and r.stride == 1,
    "stem_s2": lambda r, p: _stem(r) and r.stride == 2,
    "stem_s3": lambda r, p: _stem(r) and r.stride == 3,
    "stem_s4": lambda r, p: _stem(r) and r.stride == 4,
    "stem_ni<=8": lambda r, p: _stem(r) and _ni(p) <= 8,
    "stem_ni>8": lambda r, p: _stem(r) and _ni(p) > 8,
    "stem_units>512": lambda r, p: _stem(r) and p.IHT * ((r.W + 3) // 4) > 512,     # a second pass of the staging loop
    # weights (these also choose what the GPU tests draw)
    "s1": lambda r, p: True, "s2": lambda r, p: True, "s3": lambda r, p: True, "s4": lambda r, p: True,
    "u1": lambda r, p: True, "u2": lambda r, p: True, "u3": lambda r, p: True, "u4": lambda r, p: True,
    "u8": lambda r, p: True, "s8": lambda r, p: True,
    "per_tensor": lambda r, p: True,
    "nobias": lambda r, p: True,
    "zw0": lambda r, p: True,
    "zw_tile_mix": lambda r, p: p.n_oc_tiles >= 2,
}

_R = lambda *a: Row(*a)
ROWS = [
    # ---- conv_f32_mfma_kernel<2,2,2,1> ----
    _R(1, 8, 8, 4, 64, 3, 3, 1, 1, "M2x2x2", "w=4 ic=8 halo_small pix%8 s8"),
    _R(2, 27, 12, 17, 40, 1, 3, 2, 1, "M2x2x2", "gi 1x3 rowmul!=colmul w%4=1 ic%16>8 oc%32 oc_ragged scalar_stores u4"),
    _R(3, 8, 31, 31, 40, 1, 1, 4, 0, "M2x2x2", "gi gi_ragged w%4=3 ic=8 oc_ragged"),
    _R(2, 17, 31, 28, 24, 3, 3, 3, 1, "M2x2x2", "row_ragged row_tiles ic%16<8 oc<32 s4"),
    _R(1, 8, 6, 6, 70, 3, 3, 1, 1, "M2x2x2", "zw_tile_mix oc_ragged w%4=2"),
    _R(2, 64, 29, 29, 64, 1, 1, 3, 0, "M2x2x2", "1x1s3_nopad w%4=1 halo_small s3"),
    # ---- <2,2,2,2> ----
    _R(3, 75, 9, 11, 40, 1, 1, 2, 1, "M2x2x2S2", "gi 1x1s2_pad ng_odd_s2 ic%16>8 w%4=3 oc_ragged oc%32 scalar_stores"),
    _R(2, 128, 7, 7, 130, 3, 3, 1, 1, "M2x2x2S2", "gi oc_ragged scalar_stores u8 zw_tile_mix"),
    _R(5, 64, 5, 5, 64, 1, 1, 1, 0, "M2x2x2S2", "gi w%4=1 scalar_stores s2"),
    _R(1, 64, 8, 16, 64, 1, 1, 1, 0, "M2x2x2S2", "patch_stores per_tensor"),
    # ---- <2,2,4,1> ----
    _R(7, 40, 7, 7, 96, 3, 3, 1, 1, "M2x2x4", "gi gi_ragged oc_ragged w%4=3 scalar_stores zw_tile_mix"),
    _R(1, 8, 2, 256, 8, 1, 1, 1, 0, "M2x2x4", "ow_limit ic=8 oc<32 oc_ragged row_tiles zw0"),
    _R(2, 43, 17, 19, 24, 5, 5, 1, 2, "M2x2x4", "5x5 row_ragged row_tiles ic%16>8 w%4=3 oc<32 scalar_stores u3"),
    _R(1, 16, 20, 20, 64, 3, 3, 1, 0, "M2x2x4", "pad0 patch_stores row_tiles nobias"),
    _R(9, 16, 4, 4, 8, 1, 1, 1, 0, "M2x2x4", "gi gi>8 w=4 oc<32"),
    # ---- <2,2,4,2> ----
    _R(2, 64, 14, 14, 64, 1, 1, 1, 0, "M2x2x4S2", "patch_stores w%4=2"),
    _R(9, 64, 8, 4, 48, 1, 1, 1, 0, "M2x2x4S2", "gi gi_ragged w=4 oc_ragged oc%32 u2"),
    _R(1, 80, 14, 14, 48, 1, 1, 1, 0, "M2x2x4S2", "ng_odd_s2 oc_ragged w%4=2"),
    _R(1, 64, 31, 15, 40, 1, 1, 1, 0, "M2x2x4S2", "row_ragged row_tiles oc_ragged w%4=3 scalar_stores"),
    _R(1, 64, 80, 8, 64, 1, 1, 3, 3, "M2x2x4S2", "1x1s3_pad scalar_stores"),
    # ---- <4,1,4,1> ----
    _R(2, 17, 28, 28, 130, 3, 3, 4, 1, "M4x1x4", "oc_ragged ic%16<8 zw_tile_mix stride>k"),
    _R(2, 17, 31, 28, 65, 3, 3, 3, 1, "M4x1x4", "row_ragged row_tiles oc=65 oc_ragged scalar_stores u1"),
    _R(3, 8, 31, 31, 65, 1, 1, 4, 0, "M4x1x4", "gi gi_ragged ic=8 oc=65 oc_ragged"),
    _R(1, 16, 9, 17, 128, 2, 2, 1, 0, "M4x1x4", "2x2 pad0 halo_small w%4=1 s1"),
    _R(1, 16, 8, 16, 128, 5, 5, 1, 2, "M4x1x4", "5x5 patch_stores"),
    _R(2, 64, 20, 22, 128, 7, 1, 2, 3, "M4x1x4", "7x1 rowmul!=colmul w%4=2 row_tiles zw0"),
    # ---- <4,1,4,2> ----
    _R(1, 64, 5, 5, 65, 1, 1, 1, 0, "M4x1x4S2", "oc=65 oc_ragged w%4=1 scalar_stores one_tile_slot"),
    _R(3, 70, 6, 6, 128, 1, 1, 1, 0, "M4x1x4S2", "gi ng_odd_s2 ic%16<8 w%4=2"),
    _R(1, 64, 15, 5, 65, 1, 1, 1, 3, "M4x1x4S2", "row_ragged row_tiles oc=65 oc_ragged w%4=1 scalar_stores"),
    _R(1, 64, 8, 16, 128, 1, 1, 1, 0, "M4x1x4S2", "patch_stores per_tensor nobias"),
    # ---- <4,1,7,1> ----
    _R(1, 8, 2, 224, 65, 1, 1, 1, 0, "M4x1x7", "ow_limit oc=65 oc_ragged ic=8 row_tiles"),
    _R(5, 27, 7, 7, 130, 1, 1, 1, 0, "M4x1x7", "gi gi_ragged oc_ragged ic%16>8 w%4=3 scalar_stores"),
    _R(1, 16, 17, 26, 128, 3, 1, 1, 1, "M4x1x7", "3x1 row_ragged row_tiles patch_stores w%4=2 u2"),
    _R(1, 24, 6, 40, 150, 1, 7, 1, 3, "M4x1x7", "1x7 oc_ragged oc%32 zw_tile_mix row_tiles"),
    _R(1, 80, 28, 28, 136, 1, 1, 2, 0, "M4x1x7", "1x1s2_nopad oc_ragged patch_stores"),
    # ---- <4,1,7,2> ----
    _R(3, 64, 9, 11, 65, 1, 1, 1, 0, "M4x1x7S2", "gi gi_ragged oc=65 oc_ragged w%4=3 scalar_stores"),
    _R(1, 64, 15, 28, 128, 1, 1, 1, 0, "M4x1x7S2", "row_ragged row_tiles patch_stores"),
    _R(1, 80, 14, 14, 136, 1, 1, 1, 0, "M4x1x7S2", "ng_odd_s2 oc_ragged oc%32 patch_stores s4"),
    _R(2, 64, 12, 16, 200, 1, 1, 1, 0, "M4x1x7S2", "zw_tile_mix oc_ragged oc%32"),
    # ---- conv_f32_stem_kernel<2,2,4> ----
    _R(1, 3, 12, 12, 8, 8, 8, 4, 2, "Stem2x2x4", "8x8 stem_kw8 stem_s4 stem_ic3 stem_ni<=8 oc<32 scalar_stores one_tile_slot"),
    _R(3, 1, 14, 14, 64, 5, 5, 1, 2, "Stem2x2x4", "5x5 stem_kw5 stem_s1 stem_ic1 halo_small w%4=2 u4"),
    _R(2, 2, 9, 30, 64, 3, 3, 3, 0, "Stem2x2x4", "stem_kw3 stem_s3 stem_ic2 pad0 w%4=2 scalar_stores one_tile_slot"),
    _R(2, 4, 10, 9, 40, 2, 4, 1, 1, "Stem2x2x4", "stem_kw4 stem_ic4 w%4=1 oc_ragged s3"),
    _R(1, 3, 32, 32, 64, 7, 7, 2, 3, "Stem2x2x4", "stem_kw7 stem_s2 patch_stores"),
    # ---- <2,2,7> ----
    _R(1, 3, 2, 448, 8, 1, 1, 1, 0, "Stem2x2x7", "stem_kw1 ow_limit stem_ni>8 oc<32 row_tiles zw0"),
    _R(1, 3, 20, 120, 8, 7, 7, 2, 3, "Stem2x2x7", "stem_kw7 stem_s2 stem_ic3 row_tiles row_ragged oc<32"),
    _R(2, 4, 20, 24, 48, 5, 5, 1, 2, "Stem2x2x7", "stem_ic4 stem_kw5 stem_s1 oc_ragged per_tensor"),
    _R(1, 3, 64, 64, 64, 7, 7, 2, 3, "Stem2x2x7", "stem_kw7 patch_stores stem_units>512 row_ragged u8"),
    # ---- <4,1,7> ----
    _R(1, 2, 6, 448, 130, 3, 3, 2, 1, "Stem4x1x7", "ow_limit stem_ic2 stem_kw3 oc_ragged zw_tile_mix"),
    _R(2, 3, 32, 32, 130, 3, 3, 1, 1, "Stem4x1x7", "stem_ni<=8 oc_ragged halo_small row_tiles pix>8"),
    _R(2, 1, 9, 13, 65, 7, 7, 1, 3, "Stem4x1x7", "oc=65 stem_ic1 w%4=1 scalar_stores nobias"),
    _R(1, 3, 9, 5, 128, 3, 3, 5, 1, "Stem4x1x7", "stride>k one_tile_slot"),
    _R(1, 3, 24, 128, 128, 7, 7, 2, 3, "Stem4x1x7", "patch_stores row_tiles"),
]

_F = lambda *a: a
FALLBACK = [
    # N, IC, H, W, OC, KH, KW, stride, pad, env, instance (None: the VALU kernel), note
    _F(1, 8, 9, 3, 8, 3, 3, 1, 1, None, None, "W = 3"),
    _F(1, 8, 9, 4, 8, 3, 3, 1, 1, None, "M2x2x2", "W = 4"),
    _F(1, 4, 9, 9, 8, 3, 3, 1, 1, None, "Stem2x2x4", "IC = 4: the stem kernel"),
    _F(1, 5, 9, 9, 8, 3, 3, 1, 1, None, None, "IC = 5"),
    _F(1, 7, 9, 9, 8, 3, 3, 1, 1, None, None, "IC = 7"),
    _F(1, 8, 9, 9, 8, 3, 3, 1, 1, None, "M2x2x2", "IC = 8"),
    _F(1, 3, 30, 30, 8, 8, 8, 2, 2, None, "Stem2x2x4", "KK = 64"),
    _F(1, 3, 30, 30, 8, 9, 9, 2, 2, None, None, "KK = 81"),
    _F(1, 8, 30, 30, 8, 8, 8, 2, 2, None, "M2x2x2", "KK = 64 on the main kernel"),
    _F(1, 8, 30, 30, 8, 9, 9, 2, 2, None, None, "KK = 81 on the main kernel"),
    _F(1, 4, 9, 12, 8, 9, 3, 1, 1, None, None, "IC = 4 with KH = 9: not a stem, and IC < 8"),
    _F(1, 8, 2, 256, 8, 1, 1, 1, 0, None, "M2x2x4", "OW = 256 on MT 64"),
    _F(1, 8, 2, 257, 8, 1, 1, 1, 0, None, None, "OW = 257 on MT 64"),
    _F(1, 8, 2, 224, 65, 1, 1, 1, 0, None, "M4x1x7", "OW = 224 on MT 128"),
    _F(1, 8, 2, 225, 65, 1, 1, 1, 0, None, None, "OW = 225 on MT 128"),
    _F(1, 3, 2, 448, 8, 1, 1, 1, 0, None, "Stem2x2x7", "OW = 448 on the narrow stem"),
    _F(1, 3, 2, 449, 8, 1, 1, 1, 0, None, None, "OW = 449 on the narrow stem"),
    _F(1, 3, 2, 224, 65, 1, 1, 1, 0, None, "Stem4x1x7", "OW = 224 on the wide stem"),
    _F(1, 3, 2, 225, 65, 1, 1, 1, 0, None, None, "OW = 225 on the wide stem"),
    _F(2, 64, 14, 14, 64, 1, 1, 1, 0, {"QE_F32_MFMA": "0"}, None, "QE_F32_MFMA=0"),
    _F(1, 3, 20, 24, 8, 7, 7, 2, 3, {"QE_F32_MFMA": "0"}, None, "QE_F32_MFMA=0 on a stem"),
]


def shape_of(r):
    return tuple(r[:9])


def macs(r):
    N, IC, H, W, OC, KH, KW, s, p = r[:9]
    return N * OC * ((H + 2 * p - KH) // s + 1) * ((W + 2 * p - KW) // s + 1) * IC * KH * KW


def every_instance():
    """The 11 instances launch_conv_f32 can select, in F32Kernel order."""
    return set(STEMS + MAINS)


def covered():
    return {r.instance for r in ROWS}


def claimed():
    return {e for r in ROWS for e in r.note.split()}


def rows_of(instance):
    return [r for r in ROWS if r.instance == instance]


def row_id(r):
    return "%s-%dx%dx%dx%d-oc%d-k%dx%ds%dp%d" % (r.instance, r.N, r.IC, r.H, r.W, r.OC, r.KH, r.KW, r.stride, r.pad)
