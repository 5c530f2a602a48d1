#!/usr/bin/env python3
"""Case generators of the seeded random-geometry sweeps of the FORWARD kernels: hip_conv / hip_conv_bf16 / Winograd / k1_stream / hip_conv_nhwc / hip_sgemm and the
non-conv kernels of ConvPipeFwd (boda_amd/conv_pipe.py POOL_TEMPLATE / LRN_TEMPLATE / fwd_relu / fwd_copy, boda_amd/nhwc.py nhwc_pool / nhwc_lrn and their specialised
and fused forms, nhwc_relu / nhwc_eltwise / nhwc_copy).

Generators only: pure functions of (n, seed) on np.random.default_rng that return tuples.  Nothing here imports torch or a backend, so the lists can be built and
checked without a GPU: tests/test_fwd_fuzz_cpu.py holds the one table of seeds and counts, counts the categories below on the lists as used and proves the reference
side on them; tests/test_gpu_fwd_fuzz.py runs those very lists on be=hip.  The hand-run tools (fuzz_conv.py, fuzz_nhwc.py, fuzz_pool_lrn.py, fuzz_lrn_pool_lds.py, driven
by fuzz_all.sh) take their cases from here too: same draws as before the generators moved."""
import numpy as np

CONV_FLOP_CAP = 3e9     # 2 B OH OW OC C KH KW of a conv case: the oracle runs it in well under a second
ELEMS_CAP = 200000      # elements of a pool / LRN / elementwise tensor
ALPHAS = (1e-4, 2e-2, 0.5)
LRN_SIZES = (1, 3, 5, 9, 17)


def _cdiv(a, b):
    return -(-a // b)


# ---- convolutions and sgemm
def conv_cases(n, seed, big=False):
    """n fp32 conv geometries (B, C, H, W, OC, KH, KW, S, P): kernels 1-11 (15 % non-square), strides 1-4, pads 0 .. K/2 + 1, planes up to 39, ragged channel counts;
    at most CONV_FLOP_CAP flop (big: batches of 16-64 and planes up to 59 at 4e10, for the large workgroup tiles -- a tool's mode, not in the suite)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = int(rng.choice([1, 1, 2, 3, 3, 3, 4, 5, 5, 7, 11]))
        kh, kw = (k, k) if rng.random() < 0.85 else (k, int(rng.choice([1, 2, 3, 5])))
        s = int(rng.choice([1, 1, 1, 2, 2, 3, 4]))
        p = int(rng.integers(0, max(kh, kw) // 2 + 2))
        h = int(rng.integers(max(kh - 2 * p, 1), 40)); w = int(rng.integers(max(kw - 2 * p, 1), 40))
        if h + 2 * p < kh or w + 2 * p < kw:
            continue
        if big:   # enough tiles for the 128x128 / 64x256 / 96x256 / 128x256 workgroup shapes
            b = int(rng.choice([16, 33, 64])); h = int(rng.integers(max(kh - 2 * p, 6), 60)); w = int(rng.integers(max(kw - 2 * p, 6), 60))
        else:
            b = int(rng.choice([1, 2, 3, 5, 8, 17]))
        c = int(rng.choice([1, 2, 3, 4, 7, 8, 16, 19, 32, 48, 64])); oc = int(rng.choice([1, 3, 8, 16, 24, 33, 64, 96, 100, 128, 160]))
        if 2.0 * b * ((h + 2 * p - kh) // s + 1) * ((w + 2 * p - kw) // s + 1) * oc * c * kh * kw > (4e10 if big else CONV_FLOP_CAP):
            continue
        out.append((b, c, h, w, oc, kh, kw, s, p))
    return out


def conv_mode_cases(n, seed, big, mode):
    """conv_cases filtered per mode: bf16 -- channel counts the bf16 patch kernel takes (multiples of 8) mixed with others; winograd -- 3x3 / stride 1 only;
    k1s -- 1x1 / stride 1 / no padding."""
    rng = np.random.default_rng(seed + 7)
    out = []
    for sh in conv_cases(40 * n, seed, big):
        b, c, h, w, oc, kh, kw, s, p = sh
        if mode == "winograd":
            sh = (b, c, h, w, oc, 3, 3, 1, min(p, 2))
            if h + 2 * sh[8] < 3 or w + 2 * sh[8] < 3: continue
        elif mode == "k1s":
            sh = (b, c, h, w, oc, 1, 1, 1, 0)
        elif mode == "bf16" and rng.random() < 0.6:
            sh = (b, int(rng.choice([16, 24, 32, 40, 64, 96])), h, w, oc, kh, kw, 1 if rng.random() < 0.7 else s, p)
            if (h + 2 * p - kh) < 0 or (w + 2 * p - kw) < 0: continue
        out.append(sh)
        if len(out) == n: break
    return out


def conv_bf16_cases(n, seed):
    return conv_mode_cases(n, seed, False, "bf16")


def winograd_cases(n, seed):
    return conv_mode_cases(n, seed, False, "winograd")


def k1s_specs(shapes, seed):
    """One k1_stream spec per 1x1 shape, drawn in order from one stream: WIxWJxOCBxCB of kernels/k1_stream_f32.hip, or (every other one) qWJxOCBxRING[xN] of
    kernels/k1_quad_f32.hip with RING a divisor of the K step count."""
    rng = np.random.default_rng(seed + 13)
    out = []
    for sh in shapes:
        wi, wj = [(1, 4), (2, 2), (4, 1), (1, 8), (8, 1), (1, 1), (3, 1), (2, 4)][int(rng.integers(0, 8))]
        ocb = int(rng.integers(1, 5)); cb = int(rng.integers(1, 3))
        if (sh[1] + 1) // 2 * cb + 32 * ocb * cb + 30 > 256: cb = 1
        if (sh[1] + 1) // 2 * cb + 32 * ocb * cb + 30 > 256: ocb = 1
        spec = f"{wi}x{wj}x{ocb}x{cb}"
        if rng.random() < 0.5:   # the 16-bytes-per-lane kernel: planes of >= 4 pels
            ks = (sh[1] + 1) // 2; divs = [d for d in range(1, 17) if ks % d == 0]
            spec = f"q{int(rng.choice([1, 2, 4, 8]))}x{int(rng.integers(1, 4))}x{int(rng.choice(divs))}" + (f"x{int(rng.integers(1, 3))}" if rng.random() < 0.5 else "")
        out.append(spec)
    return out


def k1s_cases(n, seed, big=False):
    """n cases (shape, spec): a 1x1 / stride-1 geometry with its drawn k1_stream spec (a spec the kernel does not take for the shape is refused as an unsupported configuration)."""
    shapes = conv_mode_cases(n, seed, big, "k1s")
    return list(zip(shapes, k1s_specs(shapes, seed)))


NHWC_TILES = ["", "", "", "128x128x0x4x1", "64x256x0x2x2", "64x128x0x2x2", "128x64x0x4x1", "32x128x0x1x4", "256x128x0x4x1x1", "64x64x0x2x2", "128x256x0x4x2x1"]


def nhwc_conv_draws(seed):
    """The endless stream of channels-last bf16 conv draws (shape, forced tile or "", float output?): kernels 2-7 with more than one tap, stride 1 (15 %: 2),
    channel counts around the 8-channel chunk, at most CONV_FLOP_CAP flop.  (The tool skips a draw whose forced tile the layer's kernel refuses, so it takes as many as it needs.)"""
    rng = np.random.default_rng(seed)
    while True:
        k = int(rng.choice([2, 3, 3, 3, 4, 5, 5, 7])); kh, kw = (k, k) if rng.random() < 0.8 else (k, int(rng.choice([1, 2, 3, 5])))
        if kh * kw < 2: continue
        p = int(rng.integers(0, max(kh, kw) // 2 + 2)); s = 1 if rng.random() < 0.85 else 2
        b = int(rng.choice([1, 2, 3, 5, 9, 17, 40])); h = int(rng.integers(max(kh - 2 * p, 1), 34)); w = int(rng.integers(max(kw - 2 * p, 1), 34))
        c = int(rng.choice([3, 8, 16, 24, 32, 40, 56, 64, 72, 96, 136])); oc = int(rng.choice([1, 8, 16, 24, 33, 48, 64, 96, 100, 128, 160, 208]))
        if h + 2 * p < kh or w + 2 * p < kw: continue
        if 2.0 * b * ((h + 2 * p - kh) // s + 1) * ((w + 2 * p - kw) // s + 1) * oc * c * kh * kw > CONV_FLOP_CAP: continue
        tile = NHWC_TILES[int(rng.integers(0, len(NHWC_TILES)))]; f32 = bool(rng.random() < 0.5)
        yield (b, c, h, w, oc, kh, kw, s, p), tile, f32


def nhwc_conv_cases(n, seed):
    """The first n draws of nhwc_conv_draws: (shape, forced tile, float output?)."""
    g = nhwc_conv_draws(seed)
    return [next(g) for _ in range(n)]


def sgemm_cases(n, seed):
    """n (M, N, K), each 1-300; two in five have M and N rounded up to multiples of 4 (the float4 loader modes)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        M, N, K = (int(rng.integers(1, 301)) for _ in range(3))
        if rng.random() < 0.4:
            M, N = min(300, 4 * (M // 4 + 1)), min(300, 4 * (N // 4 + 1))
        out.append((M, N, K))
    return out


def conv_categories(case):
    """What a conv geometry (B, C, H, W, OC, KH, KW, S, P) exercises, by name: non_square (KH != KW), k1 (a 1x1 kernel), strided, padded, pad_ge_k (a window wholly
    in the padding on an axis: P >= K), one_out (OH or OW of 1), c_ragged (C % 8), oc_ragged (OC % 8), tail ((H + 2P - KH) % S: columns behind the last window)."""
    B, C, H, W, OC, KH, KW, S, P = case
    OH, OW = (H + 2 * P - KH) // S + 1, (W + 2 * P - KW) // S + 1
    cats = set()
    if KH != KW: cats.add("non_square")
    if KH * KW == 1: cats.add("k1")
    if S > 1: cats.add("strided")
    if P: cats.add("padded")
    if P >= KH or P >= KW: cats.add("pad_ge_k")
    if OH == 1 or OW == 1: cats.add("one_out")
    if C % 8: cats.add("c_ragged")
    if OC % 8: cats.add("oc_ragged")
    if (H + 2 * P - KH) % S or (W + 2 * P - KW) % S: cats.add("tail")
    return cats


# ---- pooling, LRN and their pairs
def pool_out_hw(H, W, kern, stride, pad):
    """The reference's ceil rule (src/conv_util.cc:198-204): a padded plane below the window on EITHER axis gives 1 x 1."""
    if H + 2 * pad[0] < kern[0] or W + 2 * pad[1] < kern[1]:
        return 1, 1
    return _cdiv(H + 2 * pad[0] - kern[0], stride[0]) + 1, _cdiv(W + 2 * pad[1] - kern[1], stride[1]) + 1


def pool_geom(case):
    """-> (kern, stride, pad, OH, OW) with a global pooling (kern None) resolved as ConvPipe.add does."""
    B, C, H, W, kern, stride, pad, avg = case
    if kern is None:
        kern, stride, pad = (H, W), (1, 1), (0, 0)
    return (kern, stride, pad) + pool_out_hw(H, W, kern, stride, pad)


def empty_windows(case):
    """How many output rows and columns have a window that lies wholly in the padding -> (rows, cols)."""
    B, C, H, W = case[:4]
    kern, stride, pad, OH, OW = pool_geom(case)
    rows = sum(1 for oy in range(OH) if min(H, oy * stride[0] - pad[0] + kern[0]) <= max(0, oy * stride[0] - pad[0]))
    cols = sum(1 for ox in range(OW) if min(W, ox * stride[1] - pad[1] + kern[1]) <= max(0, ox * stride[1] - pad[1]))
    return rows, cols


def chan_categories(C):
    """c_mod8 (C % 8 != 0: pad channels), c_le8 (one 16-byte chunk), c_16 (two chunks), chunks_odd (a chunk count that does not divide the wave's 64 lanes)."""
    cats = set()
    if C % 8: cats.add("c_mod8")
    if C <= 8: cats.add("c_le8")
    if C == 16: cats.add("c_16")
    if 64 % _cdiv(C, 8): cats.add("chunks_odd")
    return cats


POOL_CATS = ("kh_ne_kw", "sy_ne_sx", "py_ne_px", "h_ne_w", "stride_gt_win", "win_gt_plane", "empty", "global", "taps_gt_64", "ow_mod4", "ow_lt4", "max", "avg",
             "c_mod8", "c_le8", "c_16", "chunks_odd")


def pool_categories(case):
    """The branches a pooling case (B, C, H, W, kern or None, stride, pad, avg) reaches, by name (POOL_CATS): unequal window / stride / padding / plane sides; a stride
    above the window; a window above the plane on an axis; at least one window wholly in the padding (the `nonempty` fallbacks of conv_pipe.py and nhwc.py); global
    pooling; more than 64 taps (the generic forms); OW % 4 and OW < 4 (the XT tail of nhwc.POOL_SPEC_SRC); max / avg; and chan_categories."""
    B, C, H, W, kern0, stride0, pad0, avg = case
    kern, stride, pad, OH, OW = pool_geom(case)
    cats = chan_categories(C)
    if kern[0] != kern[1]: cats.add("kh_ne_kw")
    if stride[0] != stride[1]: cats.add("sy_ne_sx")
    if pad[0] != pad[1]: cats.add("py_ne_px")
    if H != W: cats.add("h_ne_w")
    if stride[0] > kern[0] or stride[1] > kern[1]: cats.add("stride_gt_win")
    if kern[0] > H or kern[1] > W: cats.add("win_gt_plane")
    if sum(empty_windows(case)): cats.add("empty")
    if kern0 is None: cats.add("global")
    if kern[0] * kern[1] > 64: cats.add("taps_gt_64")
    if OW % 4: cats.add("ow_mod4")
    if OW < 4: cats.add("ow_lt4")
    cats.add("avg" if avg else "max")
    return cats


_POOL_CHANS = [1, 3, 5, 8, 12, 16, 17, 24, 32, 40, 56, 64]
_POOL_WANT = ["empty", "stride_gt_win", "global", "taps_gt_64", "win_gt_plane", "ow_lt4", "c_le8", "c_16", "chunks_odd", "py_ne_px", "sy_ne_sx", "empty"]


def _pool_draw(rng, want):
    B = int(rng.choice([1, 2, 3, 5])); C = int(rng.choice(_POOL_CHANS))
    H, W = int(rng.integers(1, 31)), int(rng.integers(1, 31))
    if rng.random() < 0.25: W = H
    kh = int(rng.choice([1, 2, 3, 3, 4, 5, 7])); kw = kh if rng.random() < 0.5 else int(rng.choice([1, 2, 3, 5, 6]))
    sy = int(rng.choice([1, 1, 2, 2, 3, 4])); sx = sy if rng.random() < 0.5 else int(rng.choice([1, 2, 3, 4]))
    py = int(rng.integers(0, kh)); px = py if (rng.random() < 0.5 and py < kw) else int(rng.integers(0, kw))
    if want not in ("empty", "stride_gt_win", None):     # (strides above the window, and the empty windows they bring, have slots of their own)
        sy, sx = min(sy, kh), min(sx, kw)
    kern = (kh, kw)
    if want == "empty":            # a last window wholly in the padding: a stride at or above the window and a padding (H 3, k 2, s 2, p 1 gives three rows, the last one empty)
        kh = int(rng.integers(2, 4)); sy = int(rng.integers(kh, 5)); py = int(rng.integers(1, kh)); H = int(rng.integers(1, 12)); kern = (kh, kw)
    elif want == "stride_gt_win":
        kh = int(rng.integers(1, 4)); sy = int(rng.integers(kh + 1, 5)); py = int(rng.integers(0, kh)); kern = (kh, kw)
    elif want == "global":
        kern = None; H, W = int(rng.integers(1, 13)), int(rng.integers(1, 13)); sy = sx = 1; py = px = 0
    elif want == "taps_gt_64":
        kh, kw = int(rng.integers(8, 12)), int(rng.integers(7, 12)); kern = (kh, kw); H, W = int(rng.integers(kh, 31)), int(rng.integers(kw, 31)); C = int(rng.choice(_POOL_CHANS[:8]))
        py, px = int(rng.integers(0, 4)), int(rng.integers(0, 4))
    elif want == "win_gt_plane":
        kh = int(rng.integers(3, 8)); kern = (kh, kw); H = int(rng.integers(1, kh)); py = int(rng.integers(0, kh))
    elif want == "ow_lt4":
        W = int(rng.integers(1, 3 * sx + 1))
    elif want == "c_le8":
        C = int(rng.choice([1, 2, 3, 5, 7, 8]))
    elif want == "c_16":
        C = 16
    elif want == "chunks_odd":
        C = int(rng.choice([17, 20, 24, 33, 40, 41, 56]))
    elif want == "sy_ne_sx":       # unequal strides at or below the window: every window meets the plane, so the specialised forms take it
        kh, kw = int(rng.integers(2, 6)), int(rng.integers(3, 6)); kern = (kh, kw); sy = int(rng.integers(1, kh + 1)); sx = sy % kw + 1; py, px = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        H, W = int(rng.integers(kh, 31)), int(rng.integers(kw, 31))
    elif want == "py_ne_px":
        kh, kw = int(rng.integers(2, 6)), int(rng.integers(2, 6)); kern = (kh, kw); py = int(rng.integers(0, kh)); px = (py + 1) % kw
    return (B, C, H, W, kern, (sy, sx), (py, px), 0)


def pool_cases(n, seed):
    """n pooling cases (B, C, H, W, kern or None, (SY, SX), (PY, PX), avg).  Planes 1-30, windows 1-7 (half of them non-square), strides 1-4 (half unequal),
    paddings below the window on each axis (half unequal), channel counts around the 8-channel chunk; at most ELEMS_CAP input elements.  Every case
    is bent towards one category of pool_categories in turn (_POOL_WANT; drawn again until it holds).  The average flag alternates from case to case (and the other
    way round in the next twelve), so that the two `empty` slots of a twelve are one maximum and one average; the global pooling is an average first."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        want = _POOL_WANT[len(out) % len(_POOL_WANT)]
        for _ in range(2000):
            case = _pool_draw(rng, want)
            case = case[:7] + ((len(out) + len(out) // 12) % 2,) if want != "global" else case[:7] + (1 - (len(out) // 12) % 2,)
            if case[0] * case[1] * case[2] * case[3] > ELEMS_CAP:
                continue
            cats = pool_categories(case)
            if want is None or (want in cats and (want != "sy_ne_sx" or "empty" not in cats)):
                break
        else:
            raise RuntimeError(f"pool_cases: no draw reached category {want}")
        out.append(case)
    return out


def lrn_straddles(case):
    """A position count that is not a multiple of the wave size at a chunk count where a position's chunks straddle a wave edge (chunks do not divide 64, and the
    tensor has more chunks than one wave)."""
    B, C, H, W = case[:4]
    c8 = _cdiv(C, 8)
    return bool(64 % c8) and (B * H * W) % 64 != 0 and B * H * W * c8 > 64


def lrn_categories(case):
    """The branches an LRN case (B, C, H, W, local_size, alpha, beta, k) reaches: ls_<n> for the window sizes of LRN_SIZES, ls_gt_c (a window larger than the channel
    count), ls_even, alpha_<a> for ALPHAS, straddle (lrn_straddles), and chan_categories."""
    B, C, H, W, ls, alpha, beta, k = case
    cats = chan_categories(C)
    if ls in LRN_SIZES: cats.add(f"ls_{ls}")
    if ls > C: cats.add("ls_gt_c")
    if ls % 2 == 0: cats.add("ls_even")
    for a in ALPHAS:
        if alpha == a: cats.add(f"alpha_{a:g}")
    if lrn_straddles(case): cats.add("straddle")
    return cats


LRN_CATS = tuple(f"ls_{n}" for n in LRN_SIZES) + ("ls_gt_c", "ls_even") + tuple(f"alpha_{a:g}" for a in ALPHAS) + ("straddle", "c_mod8", "c_le8", "c_16", "chunks_odd")
# slot of every twelve -> (local_size, the channel counts to draw from)
_LRN_SLOTS = [(1, [8, 16, 64]), (3, [16]), (5, [1, 2, 3, 4]), (9, [17, 24, 40, 56]), (17, [9, 12, 15]), (4, [3, 16, 20, 40]), (2, [1, 5, 8]), (3, [20, 24, 36, 40, 56]),
              (17, [32, 70]), (9, [5, 8]), (5, None), (6, None)]


def lrn_cases(n, seed):
    """n LRN cases (B, C, H, W, local_size, alpha, beta, k): each twelve walk _LRN_SLOTS -- local_size 1 / 3 / 5 / 9 / 17, the even 2 / 4 / 6, windows above the channel
    count, one and two chunks, chunk counts that do not divide 64 (slot 7 on a position count that straddles a wave edge) --, alpha walks ALPHAS (shifted by one every
    twelve), beta from {0.5, 0.75, 1.0}, k from {1, 2}; planes 1 x 1 to 12 x 12, at most ELEMS_CAP elements."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        ls, chans = _LRN_SLOTS[i % 12]
        C = int(rng.choice(chans)) if chans else int(rng.integers(1, 71))
        B, H, W = int(rng.choice([1, 2, 3, 5])), int(rng.integers(1, 13)), int(rng.integers(1, 13))
        case = (B, C, H, W, ls, ALPHAS[(i + i // 12) % 3], float(rng.choice([0.5, 0.75, 1.0])), float(rng.choice([1.0, 2.0])))
        if i % 12 == 7 and not lrn_straddles(case):
            continue
        out.append(case)
    return out


def pool_lrn_pair_cases(n, seed):
    """n pairs (B, C, H, W, lrn_first, (kern, stride, pad), (local_size, alpha, beta, k)) of a max pooling and an LRN that a ConvPipe chains, alternating order
    (even index: LRN -> Pooling).  Windows 2-5 (a fifth non-square), strides 1-3 (a quarter unequal), padding on four in ten; local_size 3-9, odd; channel counts in
    whole chunks mostly (what the fused kernels take), one in six not; planes 3-24; every window meets the plane."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        B = int(rng.choice([1, 2, 3])); C = int(rng.choice([8, 16, 24, 40, 64, 96])) if len(out) % 6 != 5 else int(rng.choice([3, 12, 20]))
        H, W = int(rng.integers(3, 25)), int(rng.integers(3, 25))
        kh = int(rng.choice([2, 3, 3, 3, 4, 5])); kw = kh if rng.random() < 0.8 else int(rng.choice([1, 2, 3, 5]))
        sy = int(rng.choice([1, 2, 2, 2, 3])); sx = sy if rng.random() < 0.75 else int(rng.choice([1, 2, 3]))
        pd = (int(rng.integers(0, kh)), int(rng.integers(0, kw))) if rng.random() < 0.4 else (0, 0)
        if kh > H + 2 * pd[0] or kw > W + 2 * pd[1] or B * C * H * W > ELEMS_CAP or sum(empty_windows((B, C, H, W, (kh, kw), (sy, sx), pd, 0))):
            continue      # (an empty window's -FLT_MAX is -inf in bf16, and an LRN over it is Inf - Inf in the oracle's carried sum: pool_cases hold the empty windows)
        lrn = (int(rng.choice([3, 5, 5, 7, 9])), float(rng.choice(ALPHAS)), float(rng.choice([0.75, 0.5])), float(rng.choice([1.0, 2.0])))
        out.append((B, C, H, W, int(len(out) % 2 == 0), ((kh, kw), (sy, sx), pd), lrn))
    return out


def elementwise_cases(n, seed):
    """n cases (B, chans, H, W): three channel counts for a three-input Concat, unequal, multiples of 8 (the channels-last Concat refuses others); the first one is
    also the tensor of the stand-alone ReLU and of the Eltwise with and without a ReLU.  The plane size takes the residues 0-3 mod 4 in turn (fwd_copy / fwd_relu
    run on flat indices); at most ELEMS_CAP elements in the Concat output."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        H, W = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        if (H * W) % 4 != len(out) % 4:
            continue
        chans = tuple(int(c) for c in rng.choice([8, 16, 24, 32, 40, 48], 3, replace=False))
        B = int(rng.choice([1, 2, 3, 5]))
        if B * sum(chans) * H * W > ELEMS_CAP:
            continue
        out.append((B, chans, H, W))
    return out


# ---- the pipes of the hand-run tools (tools/fuzz_pool_lrn.py, tools/fuzz_lrn_pool_lds.py): (B, C, H, W, ops) with ops as
#      ("Pooling", tag, bottom, kern, stride, pad, avg) / ("LRN", tag, bottom, (local_size, alpha, beta, k))
def pool_lrn_pipes(n, seed):
    """n pipes of up to ten poolings and three LRNs (3, 5, 7), every op reading the input node."""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        B = int(rng.choice([1, 2, 5])); C = int(rng.choice([8, 24, 40, 64, 16, 32])); H = int(rng.integers(3, 30)); W = int(rng.integers(3, 30))
        r = np.random.default_rng(seed * 1000 + it)
        ops = []; k = 0
        for _ in range(10):
            kh = int(r.choice([1, 2, 3, 3, 4, 5, 7])); kw = kh if r.random() < 0.8 else int(r.choice([1, 2, 3, 5]))
            s = int(r.choice([1, 1, 2, 2, 3])); pd = int(r.integers(0, max(1, min(kh, kw))))
            if kh > H + 2 * pd or kw > W + 2 * pd: continue
            ops.append(("Pooling", f"p{k}", "data", (kh, kw), (s, s), (pd, pd), int(r.random() < 0.4))); k += 1
        for j, ls in enumerate((3, 5, 7)):
            ops.append(("LRN", f"l{j}", "data", (ls, float(r.choice([1e-4, 2e-2, 0.5])), 0.75, float(r.choice([1.0, 2.0])))))
        out.append((B, C, H, W, ops))
    return out


def lrn_pool_pipes(n, seed):
    """n pipes of up to eight LRN -> max pooling pairs, every LRN reading the input node."""
    rng = np.random.default_rng(seed)
    out = []
    for it in range(n):
        B = int(rng.choice([1, 2, 3, 5])); C = int(rng.choice([8, 16, 24, 40, 64, 96, 192, 256])); H = int(rng.integers(3, 40)); W = int(rng.integers(3, 40))
        r = np.random.default_rng(seed * 1000 + it)
        ops = []; k = 0
        for _ in range(8):
            kh = int(r.choice([2, 3, 3, 3, 4, 5])); kw = kh if r.random() < 0.8 else int(r.choice([1, 2, 3, 5]))
            s = int(r.choice([1, 2, 2, 2, 3])); pd = int(r.integers(0, max(1, min(kh, kw)))) if r.random() < 0.4 else 0
            if kh > H + 2 * pd or kw > W + 2 * pd: continue
            ls = int(r.choice([3, 5, 5, 7, 9]))
            ops.append(("LRN", f"l{k}", "data", (ls, float(r.choice([1e-4, 2e-2, 0.5])), float(r.choice([0.75, 0.5])), float(r.choice([1.0, 2.0])))))
            ops.append(("Pooling", f"p{k}", f"l{k}", (kh, kw), (s, s), (pd, pd), 0)); k += 1
        out.append((B, C, H, W, ops))
    return out


FAMILIES = ("conv", "conv_bf16", "winograd", "k1s", "nhwc_conv", "sgemm", "pool", "lrn", "pool_lrn_pair", "elementwise")
