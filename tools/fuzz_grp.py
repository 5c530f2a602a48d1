#!/usr/bin/env python3
"""Seeded random-geometry sweeps for the grouped convolution (kernels/conv_grp_f32.hip), the Deconvolution family (kernels/deconv_f32.hip) and hip_crop / hip_crop_bck.

usage: fuzz_grp.py [n_cases] [seed] [grp|deconv|crop|all]     (GPU box; run it on its own under `timeout`)
One process, one be=hip backend.  Every case runs the checks of tests/test_gpu_grp_fuzz.py (the HIP kernel against be=cpu on the slices resp. the exchanged roles, the
filter gradients against oracle/bck_chain.py with the launched BK / KSL, everything against float64 under the project's written bounds); the grouped cases run under
the planner's choice and under every forced tile of the form they were drawn for.  A failed compare prints `MISMATCH <family> <case> <kernel cfg> <what> <how many
elements>`, the last line is the summary (cases, mismatches, the worst fraction of each float64 bound, the kernels / tile configs used) and the exit code is 1 on any
mismatch.  Anything that is not a failed compare -- an HIP error included -- ends the run at once.

The case generators and the category functions below are importable without a GPU (nothing here touches HIP at import) and are pure functions of (n, seed) on
np.random.default_rng; tests/test_grp_fuzz_cpu.py checks them and holds the checkers to their bounds on the very cases the GPU test uses.  The category functions
restate, in Python, which branch of a kernel a geometry reaches: the planner's tile rules (plan_conv_grp) and the forward Deconvolution's chunking (deconv_grid)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

import fuzz_bck
from fuzz_bck import FLOP_CAP, _cdiv

EXTS = [1, 2, 3, 5, 8, 15, 16, 17, 31, 32, 33]   # a group's in / out channels: the 8 / 16 / 32 edges of the planner and of the 16- and 32-row MFMA blocks
GROUPS = [2, 3, 4, 7]
DW_CHANS = [2, 3, 5, 8, 19, 33]                   # channel counts of the depthwise draws (g = C, channel multiplier 1, 2 or 3)

# ---- the forced tiles of the grouped functions (tests/test_gpu_conv_grp.py's sets): name -> tile, or -> a function of the case for the filter gradient's plans
FWD_DIRECT_TILES = {"vx1": "1x1x1x2x2x1x1", "vx2": "1x2x1x2x2x1x1", "vx4": "1x4x1x2x2x1x1"}
IN_DIRECT_TILES = {"vx1": "1x1x1x2x2x1x1"}
IN_VX4_TILES = {"vx4": "1x4x1x2x2x1x1"}
MATRIX_TILES = {"m32": "32x128x2x1x4x1x1", "m32x2x2": "64x128x2x1x2x1x1", "m16": "16x64x4x1x4x1x1"}   # 32-blocks, 2 x 2 of them per wave, 16-blocks


def grp_k(case):
    """K = B * OH * OW of a grouped case: the filter gradient's reduction."""
    B, g, C, OC, H, W, (KH, KW), (SY, SX), (PY, PX) = case
    return B * ((H + 2 * PY - KH) // SY + 1) * ((W + 2 * PX - KW) // SX + 1)


def bk_odd(K):
    """An odd K step that divides neither K nor 4."""
    return next(b for b in (7, 5, 9, 11, 3, 13) if K % b)


def bk_quad(K):
    """A multiple of both MFMA k steps that does not divide K (32 where every candidate does)."""
    return next((b for b in (12, 20, 28, 44) if K % b), 32)


FILTS_DIRECT_PLANS = {"d32s1": lambda K: (32, 1), "d32s2": lambda K: (32, 2), "dodd_s3": lambda K: (bk_odd(K), 3), "d4s300": lambda K: (4, 300)}
FILTS_MATRIX_PLANS = {"m32s1": lambda K: (32, 32, 32, 1), "m32s2": lambda K: (32, 32, 32, 2), "m32s3": lambda K: (32, 32, bk_quad(K), 3), "m16s3": lambda K: (16, 32, bk_quad(K), 3)}


def filts_tile(name, case):
    """The seven-field tile of a named filter-gradient plan for a case."""
    K = grp_k(case)
    if name in FILTS_DIRECT_PLANS:
        bk, ksl = FILTS_DIRECT_PLANS[name](K)
        return f"1x1x{bk}x2x2x1x{ksl}"
    bi, bj, bk, ksl = FILTS_MATRIX_PLANS[name](K)
    return f"{bi}x{bj}x{bk}x1x1x1x{ksl}"


def forced_tiles(case, func, form):
    """{name: tile} the GPU test forces on a case drawn for (func, form)."""
    if func == "filts":
        return {n: filts_tile(n, case) for n in (FILTS_MATRIX_PLANS if form == "matrix" else FILTS_DIRECT_PLANS)}
    if form == "matrix":
        return dict(MATRIX_TILES)
    return dict(FWD_DIRECT_TILES if func == "fwd" else IN_VX4_TILES if form == "direct_vx4" else IN_DIRECT_TILES)


def slice_ends(K, bk, ksl):
    """[(k0, k1)] of the KSL slices of whole BK steps, clipped to K (the kernels' kt_per rule; oracle/bck_chain.filts_slices)."""
    nkt = _cdiv(K, bk)
    per = _cdiv(nkt, ksl)
    return [(min(min(s * per, nkt) * bk, K), min(min(min(s * per, nkt) + per, nkt) * bk, K)) for s in range(ksl)]


def grp_categories(case, func, form, tile=""):
    """The branches of conv_grp_f32.hip a grouped case reaches, by name.  func: "fwd" | "in" | "filts"; form: "direct" | "direct_vx4" (the data gradient's VX = 4) |
    "matrix"; tile: a forced seven-field tile, or "" = under any of the tiles the GPU test forces on the case (forced_tiles).
    direct forward       aligned_span (SX == 1 and W % 4 == 0: VX = 4 reads the span as aligned 16-byte loads) with aligned_span_p0 .. p3 = PX % 4, wide_span (an aligned
                         span of more than two quads), ragged_quad (OW % 4 != 0), vec_store (OW % 4 == 0), narrow (OW < 3: the planner's VX = OW)
    direct data gradient vec_store (W % 4 == 0), unreached (KH < SY or KW < SX), and a, c, d, g of fuzz_bck.conv_categories on the slice
    direct filter grad.  quads (OW % 4 == 0), split_quad (quads, more than one tap, KSL > 1, BK % 4 != 0 and a slice that ends inside K off a quad boundary),
                         taps49 (7 x 7), empty_slices (KSL above the number of K steps)
    matrix form          k_tail (the reduction -- forward CG*KH*KW, data gradient OCG*TY*TX, filter gradient B*OH*OW -- odd at MT 32 / no multiple of 4 at MT 16),
                         ragged_rows (a group's row extent no multiple of MT), one_tile_two_groups (g * rows <= 32), cols_tail (the column extent -- forward B*OH*OW,
                         filter gradient CG*KH*KW, data gradient some phase's pels -- no multiple of BJ); data gradient: e_odd, e_small, f of conv_categories on the slice"""
    B, g, C, OC, H, W, (KH, KW), (SY, SX), (PY, PX) = case
    CG, OCG = C // g, OC // g
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    K = B * OH * OW
    tiles = [tile] if tile else list(forced_tiles(case, func, form).values())
    sl = fuzz_bck.conv_categories((B, CG, H, W, OCG, KH, KW, SY, SX, PY, PX))
    cats = set()
    if form != "matrix":
        if func == "fwd":
            if SX == 1 and W % 4 == 0:
                cats |= {"aligned_span", f"aligned_span_p{PX % 4}"}
                if (4 - PX % 4) % 4 + 3 + KW > 8:
                    cats.add("wide_span")
            cats.add("vec_store" if OW % 4 == 0 else "ragged_quad")
            if OW < 3: cats.add("narrow")
        elif func == "in":
            if W % 4 == 0: cats.add("vec_store")
            if KH < SY or KW < SX: cats.add("unreached")
            cats |= sl & {"a", "c", "d", "g"}
        else:
            if OW % 4 == 0: cats.add("quads")
            if KH * KW == 49: cats.add("taps49")
            for t in tiles:
                bk, ksl = int(t.split("x")[2]), int(t.split("x")[6])
                if ksl > _cdiv(K, bk): cats.add("empty_slices")
                if OW % 4 == 0 and KH * KW > 1 and ksl > 1 and bk % 4 and any(k1 < K and k1 % 4 for _, k1 in slice_ends(K, bk, ksl)):
                    cats.add("split_quad")
        return cats
    rows = CG if func == "in" else OCG
    red = {"fwd": CG * KH * KW, "in": OCG * _cdiv(KH, SY) * _cdiv(KW, SX), "filts": K}[func]
    if g * rows <= 32: cats.add("one_tile_two_groups")
    for t in tiles:
        f = [int(v) for v in t.split("x")]
        mt = 16 if f[0] // f[3] == 16 else 32
        if red % (2 if mt == 32 else 4): cats.add("k_tail")
        if rows % mt: cats.add("ragged_rows")
        if func == "fwd" and (B * OH * OW) % f[1]: cats.add("cols_tail")
        if func == "filts" and (CG * KH * KW) % f[1]: cats.add("cols_tail")
        if func == "in":
            for ry in range(SY):
                for rx in range(SX):
                    y0, x0 = (ry - PY) % SY, (rx - PX) % SX
                    n = B * (_cdiv(H - y0, SY) if y0 < H else 0) * (_cdiv(W - x0, SX) if x0 < W else 0)
                    if n % f[1]: cats.add("cols_tail")
    if func == "in":
        cats |= sl & {"e_odd", "e_small", "f"}
    return cats


GRP_WANTS = {
    ("fwd", "direct"): ["aligned_span_p0", "aligned_span_p1", "aligned_span_p2", "aligned_span_p3", "ragged_quad", "vec_store", "narrow"],
    ("in", "direct"): ["vec_store", "unreached", "a", "c", "d", "g"],
    ("in", "direct_vx4"): ["vec_store", "unreached", "a", "c", "d", "g"],
    ("filts", "direct"): ["quads", "split_quad", "taps49", "empty_slices"],
    ("fwd", "matrix"): ["k_tail", "ragged_rows", "one_tile_two_groups", "cols_tail"],
    ("in", "matrix"): ["k_tail", "ragged_rows", "one_tile_two_groups", "cols_tail", "e_odd", "e_small", "f"],
    ("filts", "matrix"): ["k_tail", "ragged_rows", "one_tile_two_groups", "cols_tail"],
}


def _grp_draw(rng, want, func, form):
    """One draw from the ranges of grp_cases, the ranges bent towards category `want` (None: unbent)."""
    B = int(rng.integers(1, 5))
    if rng.random() < 0.3:   # depthwise: g = C, channel multiplier 1, 2 or 3
        dw = True; g = int(rng.choice(DW_CHANS)); CG, OCG = 1, int(rng.integers(1, 4))
    else:
        dw = False; g = int(rng.choice(GROUPS)); CG, OCG = int(rng.choice(EXTS)), int(rng.choice(EXTS))
    k = int(rng.integers(1, 8))
    KH, KW = (k, k) if rng.random() < 0.67 else (k, int(rng.integers(1, 8)))
    if rng.random() < 0.5:
        KH, KW = KW, KH
    s = int(rng.integers(1, 5))
    SY, SX = (s, s) if rng.random() < 0.67 else (s, int(rng.integers(1, 5)))
    if rng.random() < 0.5:
        SY, SX = SX, SY
    H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    if form == "direct_vx4":
        SX = 1
    PX = None
    if want and want.startswith("aligned_span_p"):   # stride 1 in x, rows of whole quads, the pad's residue
        sq = KH == KW
        r = int(want[-1]); SX = 1; W = 4 * int(rng.integers(1, 7)); KW = int(rng.integers(r + 1, 8)); PX = int(rng.choice([p for p in range(KW) if p % 4 == r]))
        KH = KW if sq else KH   # (a square draw stays square)
    elif want == "narrow":
        W = int(rng.integers(1, 6)); SX = int(rng.integers(1, 5))
    elif want == "taps49":
        KH = KW = 7; CG, OCG = min(CG, 8), min(OCG, 8)
    elif want == "empty_slices":   # few K steps
        B = 1; H, W = int(rng.integers(1, 6)), int(rng.integers(1, 6))
    elif want in ("quads", "split_quad"):
        KH, KW = max(KH, 2), max(KW, 1)
    elif want == "unreached":
        KH = int(rng.integers(1, 4)); SY = int(rng.integers(KH + 1, 5))
    elif want == "a":
        SY = int(rng.integers(2, 5)); H = int(rng.integers(1, SY))
    elif want == "c":
        SY = int(rng.integers(1, 4)); KH = int(rng.integers(SY + 1, 8))
    elif want == "one_tile_two_groups":
        g = int(rng.choice([2, 3, 4])); CG, OCG = int(rng.choice(EXTS[:5])), int(rng.choice(EXTS[:5]))
    elif want in ("e_odd", "e_small"):
        OCG = int(rng.choice([1, 3] if dw else [1, 3, 5])); KH, KW = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    elif want == "f":
        B = int(rng.integers(3, 5)); H, W = int(rng.integers(16, 25)), int(rng.integers(16, 25)); SY, SX = int(rng.integers(1, 3)), (1 if form == "direct_vx4" else int(rng.integers(1, 3)))
        CG, OCG = min(CG, 8), min(OCG, 8)
    PY = int(rng.integers(0, KH))
    if PX is None:
        PX = int(rng.integers(0, KW))
    if want == "c":
        PY = int(rng.integers(SY, KH))
    elif want == "g":
        H = int(rng.integers(max(1, KH - 2 * PY), max(1, KH - 2 * PY) + SY))
    elif want in ("vec_store", "quads", "split_quad"):   # an extent of whole quads: the forward's / the filter gradient's OW, the data gradient's W
        if func == "in":
            W = 4 * int(rng.integers(1, 7))
        else:
            OW = 4 * int(rng.integers(1, 4)); W = (OW - 1) * SX + KW - 2 * PX + int(rng.integers(0, SX))
    return (B, g, g * CG, g * OCG, H, W, (KH, KW), (SY, SX), (PY, PX))


def grp_cases(n, seed, func, form):
    """n grouped geometries (B, g, C, OC, H, W, (KH, KW), (SY, SX), (PY, PX)) for function `func` ("fwd" | "in" | "filts") in form `form` ("direct" | "matrix", and
    "direct_vx4" for the data gradient's four-outputs-a-thread tile, which draws SX == 1 only).  B 1-4; g from GROUPS, or depthwise (g = C from DW_CHANS, channel
    multiplier 1-3); per-group extents from EXTS; KH, KW 1-7, about a third non-square; SY, SX 1-4, about a third unequal; PY, PX 0 .. kernel-1 each; H, W 1-24.  A draw
    is rejected only where the op is refused (H + 2 PY < KH, W < 1, likewise in x) or where it is too large for be=cpu (2 B OH OW OC CG KH KW > FLOP_CAP).  Seven of every
    eight cases are bent towards one of the categories GRP_WANTS[func, form] in turn (drawn again until the category holds)."""
    rng = np.random.default_rng(seed)
    wants = GRP_WANTS[(func, form)]
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else wants[(i - i // 8) % len(wants)]
        for _ in range(4000):
            case = _grp_draw(rng, want, func, form)
            B, g, C, OC, H, W, (KH, KW), (SY, SX), (PY, PX) = case
            if H < 1 or W < 1 or W > 24 or H + 2 * PY < KH or W + 2 * PX < KW:
                continue
            OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
            if 2.0 * B * OH * OW * OC * (C // g) * KH * KW > FLOP_CAP:
                continue
            if want is None or want in grp_categories(case, func, form):
                break
        else:
            raise RuntimeError(f"grp_cases: no draw reached category {want} of {func} / {form}")
        out.append(case)
    return out


# ---- Deconvolution
DECONV_CHANS = [1, 2, 3, 5, 8, 21, 33]
LDS_FLOATS = 8192   # the forward's staged filter rows (kernels/deconv_f32.hip: kLdsFloats)


def deconv_out_plane(case):
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    return (H - 1) * SY + KH - 2 * PY, (W - 1) * SX + KW - 2 * PX


def deconv_fwd_grid(case, num_cus=256):
    """deconv_grid (csrc/native_plan.cc) of the forward, restated: -> (workgroups, zs chunks, per items a chunk, items of the longest phase)."""
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    OH, OW = deconv_out_plane(case)
    items = B * _cdiv(OH, SY) * _cdiv(OW, 4)
    want = max(1, _cdiv(8 * num_cus, OC * SY))
    zs = max(1, min(want, _cdiv(items, 256)))
    return OC * SY * zs, zs, _cdiv(items, zs), items


def deconv_categories(case, num_cus=256):
    """The branches of deconv_f32.hip's forward a case reaches, by name:
    share (SX >= 4: a quad inside one stride step reads `in` once) as share47 (SX 4..7: quads that share and quads that do not) or share8 (SX >= 8); no_share (SX 1-3)
    unreached (KH < SY or KW < SX)        tap_past_kernel (KH % SY != 0 or KW % SX != 0)        empty_phase (some row phase has y0 >= OH)
    ragged_quad / vec_store (OW % 4)      rect (kernel, stride or pad unequal on the two axes)
    chunks (zs > 1)    ragged_chunk (zs > 1 and per % 256 != 0)    passes (per > 256: several passes of one workgroup)    lds_chunks (C * TY * KW > 8192 floats: kNC > 1)"""
    B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
    OH, OW = deconv_out_plane(case)
    _, zs, per, _ = deconv_fwd_grid(case, num_cus)
    cats = {"share", "share47" if SX < 8 else "share8"} if SX >= 4 else {"no_share"}
    if KH < SY or KW < SX: cats.add("unreached")
    if KH % SY or KW % SX: cats.add("tap_past_kernel")
    if any((ry - PY) % SY >= OH for ry in range(SY)): cats.add("empty_phase")
    cats.add("ragged_quad" if OW % 4 else "vec_store")
    if zs > 1: cats.add("chunks")
    if zs > 1 and per % 256: cats.add("ragged_chunk")
    if per > 256: cats.add("passes")
    if C * _cdiv(KH, SY) * KW > LDS_FLOATS: cats.add("lds_chunks")
    if KH != KW or SY != SX or PY != PX: cats.add("rect")
    return cats


DECONV_WANTS = ["share47", "share8", "no_share", "unreached", "tap_past_kernel", "empty_phase", "ragged_quad", "vec_store", "chunks", "ragged_chunk", "rect"]


def _deconv_draw(rng, want):
    B = int(rng.integers(1, 5))
    C, OC = int(rng.choice(DECONV_CHANS)), int(rng.choice(DECONV_CHANS))
    k = 64 if rng.random() < 0.04 else int(rng.integers(1, 17))
    KH, KW = (k, k) if rng.random() < 0.67 else (k, int(rng.integers(1, 17)))
    if rng.random() < 0.5:
        KH, KW = KW, KH
    s = int(rng.choice([16, 32])) if rng.random() < 0.06 else int(rng.integers(1, 9))
    SY, SX = (s, s) if rng.random() < 0.67 else (s, int(rng.integers(1, 9)))
    if rng.random() < 0.5:
        SY, SX = SX, SY
    H, W = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    if want == "share47":
        SX = int(rng.integers(4, 8))
    elif want == "share8":
        SX = int(rng.choice([8, 8, 16, 32]))
    elif want == "no_share":
        SX = int(rng.integers(1, 4))
    elif want == "unreached":
        SY = int(rng.integers(2, 9)); KH = int(rng.integers(1, SY))
    elif want == "empty_phase":   # a plane shorter than the stride
        H = 1; SY = int(rng.integers(2, 9)); KH = int(rng.integers(1, SY))
    elif want in ("chunks", "ragged_chunk"):   # more than 256 (img, row, quad) items in a phase
        B = int(rng.integers(3, 5)); H, W = int(rng.integers(6, 9)), int(rng.integers(6, 9)); SX = int(rng.integers(5, 9)); C, OC = int(rng.choice(DECONV_CHANS[:5])), int(rng.choice(DECONV_CHANS[:5]))
    PY, PX = int(rng.integers(0, KH)), int(rng.integers(0, KW))
    if want == "empty_phase":
        PY = 0
    return (B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX))


def deconv_cases(n, seed):
    """n Deconvolution geometries (B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX)), tests/deconv_ref.py's format.  B 1-4; C, OC from DECONV_CHANS; KH, KW 1-16 (now and
    then 64), about a third non-square; SY, SX 1-8 (now and then 16 or 32), about a third unequal; pads below the kernel; H, W 1-8.  A draw is rejected only where the op
    is refused (OH < 1 or OW < 1) or too large for be=cpu (2 B C H W OC KH KW > FLOP_CAP).  Seven of every eight cases are bent towards one of DECONV_WANTS in turn.  The
    categories `passes` and `lds_chunks` lie outside these ranges: tests/test_grp_fuzz_cpu.py adds hand-made cases for them."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else DECONV_WANTS[(i - i // 8) % len(DECONV_WANTS)]
        for _ in range(4000):
            case = _deconv_draw(rng, want)
            B, C, H, W, OC, (KH, KW), (SY, SX), (PY, PX) = case
            OH, OW = deconv_out_plane(case)
            if OH < 1 or OW < 1 or 2.0 * B * C * H * W * OC * KH * KW > FLOP_CAP:
                continue
            if want is None or want in deconv_categories(case):
                break
        else:
            raise RuntimeError(f"deconv_cases: no draw reached category {want}")
        out.append(case)
    return out


# ---- Crop
CROP_KINDS = ["offset0", "whole_plane", "one_pel", "quads", "ragged", "far_edge"]


def crop_kinds(case):
    B, C, H, W, OH, OW, oy, ox = case
    kinds = {"quads" if OW % 4 == 0 else "ragged"}
    if (oy, ox) == (0, 0): kinds.add("offset0")
    if (OH, OW) == (H, W): kinds.add("whole_plane")
    if (OH, OW) == (1, 1): kinds.add("one_pel")
    if oy + OH == H and ox + OW == W and (oy or ox): kinds.add("far_edge")
    return kinds


def crop_cases(n, seed):
    """n Crop windows (B, C, H, W, OH, OW, oy, ox): planes 1-24, B 1-3, C 1-5; by turns offset 0, the window equal to the plane, a window of one pel, a window of whole
    quads, a ragged one, a window against the far edge of both axes."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        kind = CROP_KINDS[len(out) % len(CROP_KINDS)]
        B, C, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 6)), int(rng.integers(1, 25)), int(rng.integers(1, 25))
        OH, OW = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        if kind == "whole_plane":
            OH, OW = H, W
        elif kind == "one_pel":
            OH, OW = 1, 1
        elif kind == "quads":
            W = max(W, 4); OW = 4 * int(rng.integers(1, W // 4 + 1))
        elif kind == "ragged":
            OW = OW + 1 if OW % 4 == 0 and OW < W else OW
        oy, ox = int(rng.integers(0, H - OH + 1)), int(rng.integers(0, W - OW + 1))
        if kind == "offset0":
            oy, ox = 0, 0
        elif kind == "far_edge":
            H, W = max(H, 2), max(W, 2); OH, OW = min(OH, H - 1), min(OW, W - 1); oy, ox = H - OH, W - OW
        case = (B, C, H, W, OH, OW, oy, ox)
        if kind in crop_kinds(case):
            out.append(case)
    return out


FAMILIES = ("grp", "deconv", "crop")
SEED_STEP = {"grp": 0, "deconv": 1000, "crop": 2000}   # the tool's families draw from different streams of one seed


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    fam = sys.argv[3] if len(sys.argv) > 3 else "all"
    if fam != "all" and fam not in FAMILIES:
        sys.exit(__doc__)
    import test_gpu_grp_fuzz as T   # the checks themselves
    from boda_amd.rtc import make_rtc
    hip = make_rtc("(be=hip)", 0); hip.init()
    cpu = make_rtc("(be=cpu)"); cpu.init()
    jobs = []   # (family, case, check)
    fams = FAMILIES if fam == "all" else (fam,)
    if "grp" in fams:
        for j, (func, form) in enumerate(GRP_WANTS):
            for i, case in enumerate(grp_cases(n, seed + SEED_STEP["grp"] + j, func, form)):
                for name, tile in [("planner", "")] + sorted(forced_tiles(case, func, form).items()):
                    jobs.append((f"grp {func} {form} {name}", case, lambda case=case, func=func, tile=tile, s=seed + i: T.check_grp_case(hip, cpu, case, s, func, tile)))
    if "deconv" in fams:
        for i, case in enumerate(deconv_cases(n, seed + SEED_STEP["deconv"])):
            jobs.append(("deconv", case, lambda case=case, s=seed + i: T.check_deconv_case(hip, cpu, case, s)))
    if "crop" in fams:
        for i, case in enumerate(crop_cases(n, seed + SEED_STEP["crop"])):
            jobs.append(("crop", case, lambda case=case, s=seed + i: T.check_crop_case(hip, case, s)))
    bad = 0
    try:
        for f, case, chk in jobs:
            try:
                chk()
            except T.Mismatch as e:   # a failed compare; every other exception (an HIP error included) ends the run
                bad += 1
                print("MISMATCH", f, case, e.cfg, e.what, e.count, "of", e.size, flush=True)
    finally:
        hip.close(); cpu.close()
    worst = ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items()))
    print(f"fuzz_grp {fam} seed={seed}: {len(jobs)} checks, {bad} mismatches; worst fraction of each float64 bound: {worst}; "
          "kernels / tile configs used:", dict(sorted(T.USED.items(), key=lambda kv: -kv[1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
