#!/usr/bin/env python3
"""Seeded random-geometry sweeps for the backward kernels (kernels/bconv_in_f32.hip, bconv_filts_f32.hip, bck_ops_f32.hip and their -DZINP=1 forms).

usage: fuzz_bck.py [n_cases] [seed] [conv|pool|lrn|softmax|flat|concat|all] [hip_tile]     (GPU box; run it on its own under `timeout`)
One process, one be=hip backend.  Every case runs the checks of tests/test_gpu_bck_fuzz.py (the HIP kernel against its bit-exact twin on be=cpu / oracle/bck_chain.py and
against float64 under the project's written bounds); a failed compare prints `MISMATCH <case> <kernel cfg> <how many elements>`, the last line is the summary (cases,
mismatches, the worst fraction of each float64 bound, the kernels / tile configs used) and the exit code is 1 on any mismatch.  Anything that is not a failed compare --
an HIP error included -- ends the run at once.  `hip_tile` forces the data gradient's tile (five fields) or the filter gradient's (seven).

The case generators below are importable without a GPU (nothing here touches HIP at import) and are pure functions of (n, seed) on np.random.default_rng;
tests/test_bck_fuzz_cpu.py checks them and holds the checkers to their bounds on the very cases the GPU test uses."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

CHANS = [1, 2, 3, 5, 8, 31, 32, 33, 63, 64, 65, 70, 129, 130]   # straddles the channel tiles (32 / 64 / 128) of the data and the filter gradient
FLOP_CAP = 2e8                                                  # 2 B OH OW OC C KH KW: be=cpu's fmaf loops stay fast


def _cdiv(a, b):
    return -(-a // b)


def conv_categories(case):
    """The branches of bconv_in_f32.hip a case reaches, by name (tests/test_bck_fuzz_cpu.py counts them over the cases the GPU test uses):
    a  H < SY or W < SX            some sub-pixel phases are empty
    b  KH < SY or KW < SX          stride above the kernel: pels that no term reaches
    c  pad >= stride               on either axis
    d  (H + 2P - K) % S != 0       rows / columns behind the last window: exactly +0
    e_odd, e_small                 K = OC ceil(KH/SY) ceil(KW/SX) odd / below 16 (the MFMA eats two k per step; BK = 16); e = both at once
    f  B ceil(H/SY) ceil(W/SX) > 128   a phase has more than one pel tile
    g  OH == 1 or OW == 1"""
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = case
    OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
    K = OC * _cdiv(KH, SY) * _cdiv(KW, SX)
    cats = set()
    if H < SY or W < SX: cats.add("a")
    if KH < SY or KW < SX: cats.add("b")
    if PY >= SY or PX >= SX: cats.add("c")
    if (H + 2 * PY - KH) % SY or (W + 2 * PX - KW) % SX: cats.add("d")
    if K % 2: cats.add("e_odd")
    if K < 16: cats.add("e_small")
    if K % 2 and K < 16: cats.add("e")
    if B * _cdiv(H, SY) * _cdiv(W, SX) > 128: cats.add("f")
    if OH == 1 or OW == 1: cats.add("g")
    return cats


def _conv_draw(rng, want):
    """One draw from the ranges of conv_cases, the ranges bent towards category `want` (None: unbent)."""
    B = int(rng.integers(1, 5))
    C, OC = int(rng.choice(CHANS)), int(rng.choice(CHANS))
    k = 11 if rng.random() < 0.06 else int(rng.integers(1, 8))
    KH, KW = (k, k) if rng.random() < 0.67 else (k, int(rng.integers(1, 8)))
    if rng.random() < 0.5:
        KH, KW = KW, KH
    s = int(rng.integers(1, 5))
    SY, SX = (s, s) if rng.random() < 0.67 else (s, int(rng.integers(1, 5)))
    if rng.random() < 0.5:
        SY, SX = SX, SY
    H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
    if want == "a":      # a plane below the stride on one axis
        SY = int(rng.integers(2, 5)); H = int(rng.integers(1, SY))
        if rng.random() < 0.5:
            SX = int(rng.integers(2, 5)); W = int(rng.integers(1, SX))
    elif want == "b":    # stride above the kernel
        KH = int(rng.integers(1, 4)); SY = int(rng.integers(KH + 1, 5))
    elif want == "c":
        SY = int(rng.integers(1, 4)); KH = int(rng.integers(SY + 1, 8))
    elif want == "e":    # a short odd K
        OC = int(rng.choice([1, 3, 5])); KH = int(rng.integers(1, 4)); KW = int(rng.integers(1, 4))
    elif want == "f":    # many pels per phase, few channels so that the case stays small
        B = int(rng.integers(3, 5)); H, W = int(rng.integers(16, 25)), int(rng.integers(16, 25)); SY, SX = int(rng.integers(1, 3)), int(rng.integers(1, 3))
        C, OC = int(rng.choice(CHANS[:9])), int(rng.choice(CHANS[:9]))
    PY, PX = int(rng.integers(0, KH)), int(rng.integers(0, KW))
    if want == "c":
        PY = int(rng.integers(SY, KH))
    elif want == "g":    # one window on an axis: H + 2 PY - KH < SY
        H = int(rng.integers(max(1, KH - 2 * PY), max(1, KH - 2 * PY) + SY))
    return (B, C, H, W, OC, KH, KW, SY, SX, PY, PX)


def conv_cases(n, seed):
    """n BckConv geometries (B, C, H, W, OC, KH, KW, SY, SX, PY, PX).  B 1-4; C, OC from CHANS; KH, KW 1-7 (now and then 11), about a third non-square; SY, SX 1-4, about a
    third unequal; PY, PX 0 .. kernel-1 each; H, W 1-24.  A draw is rejected only where the op is refused (H + 2 PY < KH, likewise in x) or where it is too large for be=cpu
    (FLOP_CAP).  Seven of every eight cases are bent towards one of the categories a .. g of conv_categories in turn (drawn again until the category holds), so that each
    category makes up roughly a sixth of the list together with the draws that reach it by themselves."""
    rng = np.random.default_rng(seed)
    order = ["a", "b", "c", "d", "e", "f", "g", None]
    out = []
    while len(out) < n:
        want = order[len(out) % len(order)]
        for _ in range(1000):
            case = _conv_draw(rng, want)
            B, C, H, W, OC, KH, KW, SY, SX, PY, PX = case
            if H + 2 * PY < KH or W + 2 * PX < KW:
                continue
            OH, OW = (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1
            if 2.0 * B * OH * OW * OC * C * KH * KW > FLOP_CAP:
                continue
            if want is None or want in conv_categories(case):
                break
        else:
            raise RuntimeError(f"conv_cases: no draw reached category {want}")
        out.append(case)
    return out


def pool_cases(n, seed):
    """n pooling geometries (B, C, H, W, (KH, KW), (SY, SX), (PY, PX), avg).  Kernels 1-7, strides 1-4, pad below the kernel, planes 1-30 (one case in twelve has a plane of
    more pels than a workgroup has threads).  Every twelve cases hold, in this order from index 0: a window larger than the padded plane (a 1 x 1 output), a stride above
    the kernel on the y axis only, a global window, a pad of kernel - 1 on both axes, a plane of more than 256 pels; the rest are unbent.  avg alternates by draw; an
    average is built with emit_out_in_yx=0, as add_bck_ops does."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        slot = len(out) % 12
        B, C = int(rng.integers(1, 4)), int(rng.choice([1, 2, 3, 5, 8, 13]))
        KH, KW = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        SY, SX = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        H, W = int(rng.integers(1, 31)), int(rng.integers(1, 31))
        PY, PX = int(rng.integers(0, KH)), int(rng.integers(0, KW))
        if slot == 0:
            KH = int(rng.integers(3, 8)); PY = int(rng.integers(0, 2)); H = int(rng.integers(1, KH - 2 * PY)) if KH - 2 * PY > 1 else 1
            if H + 2 * PY >= KH:
                continue
        elif slot == 1:
            KH = int(rng.integers(1, 4)); SY = int(rng.integers(KH + 1, 5)); PY = int(rng.integers(0, KH)); SX = int(rng.integers(1, KW + 1)); SX = min(SX, 4)
        elif slot == 2:
            H, W = int(rng.integers(1, 8)), int(rng.integers(1, 8)); KH, KW, PY, PX, SY, SX = H, W, 0, 0, 1, 1
        elif slot == 3:
            PY, PX = KH - 1, KW - 1
        elif slot == 4:
            H, W = int(rng.integers(17, 31)), int(rng.integers(17, 31))
        out.append((B, C, H, W, (KH, KW), (SY, SX), (PY, PX), int(rng.integers(0, 2))))
    return out


def lrn_cases(n, seed):
    """n LRN geometries (B, C, H, W, local_size, alpha, beta, k).  local_size odd 1-15; C 1-140, by turns below the window, a multiple of 8, C = 1..7 (mod 8), unbent;
    planes 1 x 1 to 9 x 9; alpha in [1e-4, 0.1] (log-uniform); beta in {0.5, 0.75, 1.0}; k in {1, 2}."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ls = int(rng.choice([1, 3, 5, 7, 9, 11, 13, 15]))
        turn = i % 4
        if turn == 0:
            ls = max(ls, 3); C = int(rng.integers(1, ls))
        elif turn == 1:
            C = 8 * int(rng.integers(1, 18))
        elif turn == 2:
            C = min(140, 8 * int(rng.integers(0, 17)) + 1 + (i // 4) % 7)
        else:
            C = int(rng.integers(1, 141))
        B, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 10)), int(rng.integers(1, 10))
        alpha = float(np.float32(10.0 ** rng.uniform(-4, -1)))
        out.append((B, C, H, W, ls, alpha, float(rng.choice([0.5, 0.75, 1.0])), float(rng.choice([1.0, 2.0]))))
    return out


def softmax_cases(n, seed):
    """n softmax-with-loss shapes (B, C, y, x): B 1-5, C 1-1100 (every fourth case C <= 64: less than a wave).  y = x = 1 throughout: the op refuses larger planes on
    purpose (SoftmaxWithLoss reads `label` by image only, boda_amd/op.py), so the range 1-3 a spatial softmax would have is narrowed to what can be built."""
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, 6)), int(rng.integers(1, 65)) if i % 4 == 0 else int(rng.integers(1, 1101)), 1, 1) for i in range(n)]


FLAT_EDGES = [1, 2, 3, 4, 5, 1020, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5000]


def flat_cases(n, seed):
    """n cases (size, n_ins, ratio) for zero_if_non_pos, reduce and dropout.  Sizes 1-5000: the first cases walk FLAT_EDGES (1, 2, 3, multiples of 4 and of 1024 and
    those +-1) from a seeded start, the others are uniform; 2-8 reduce inputs; dropout ratios in (0, 1), 0.01 and 0.99 by turns among them."""
    rng = np.random.default_rng(seed)
    start = int(rng.integers(0, len(FLAT_EDGES)))
    out = []
    for i in range(n):
        size = FLAT_EDGES[(start + i) % len(FLAT_EDGES)] if i < len(FLAT_EDGES) else int(rng.integers(1, 5001))
        ratio = (0.01, 0.99)[(i // 3) % 2] if i % 3 == 0 else float(np.float32(rng.uniform(0.02, 0.98)))
        out.append((size, int(rng.integers(2, 9)), ratio))
    return out


def concat_cases(n, seed):
    """n concat / split cases (B, chans, H, W): 2-5 members of 1-9 channels; the plane size takes the residues 0, 1, 2, 3 mod 4 in turn, so both the quad path and the
    scalar path are taken and runs start on and off a quad."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        H, W = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        if (H * W) % 4 != len(out) % 4:
            continue
        chans = tuple(int(c) for c in rng.integers(1, 10, int(rng.integers(2, 6))))
        out.append((int(rng.integers(1, 4)), chans, H, W))
    return out


FAMILIES = ("conv", "pool", "lrn", "softmax", "flat", "concat")
SEED_STEP = {"conv": 0, "pool": 1000, "lrn": 2000, "softmax": 3000, "flat": 4000, "concat": 5000}   # the tool's families draw from different streams of one seed


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    fam = sys.argv[3] if len(sys.argv) > 3 else "all"
    tile = sys.argv[4] if len(sys.argv) > 4 else ""
    if fam != "all" and fam not in FAMILIES:
        sys.exit(__doc__)
    import test_gpu_bck_fuzz as T   # the checks themselves
    from boda_amd.rtc import make_rtc
    hip = make_rtc("(be=hip)", 0); hip.init()
    cpu = make_rtc("(be=cpu)"); cpu.init()
    fams = FAMILIES if fam == "all" else (fam,)
    tile_in = tile if tile.count("x") == 4 else ""
    tile_f = tile if tile.count("x") >= 5 else ""
    checks = {
        "conv": (conv_cases, lambda i, c: T.check_conv_case(hip, cpu, c, seed + i, tile=tile_in, ftile=tile_f)),
        "pool": (pool_cases, lambda i, c: T.check_pool_case(hip, cpu, c, i, seed + i)),
        "lrn": (lrn_cases, lambda i, c: T.check_lrn_case(hip, cpu, c, seed + i)),
        "softmax": (softmax_cases, lambda i, c: T.check_softmax_case(hip, cpu, c, seed + i)),
        "flat": (flat_cases, lambda i, c: T.check_flat_case(hip, cpu, c, seed + i)),
        "concat": (concat_cases, lambda i, c: T.check_concat_case(hip, cpu, c, seed + i)),
    }
    bad = total = 0
    try:
        for f in fams:
            gen, chk = checks[f]
            for i, case in enumerate(gen(n, seed + SEED_STEP[f])):
                total += 1
                try:
                    chk(i, case)
                except T.Mismatch as e:   # a failed compare; every other exception (an HIP error included) ends the run
                    bad += 1
                    print("MISMATCH", f, case, e.cfg, e.what, e.count, "of", e.size, flush=True)
    finally:
        hip.close(); cpu.close()
    worst = ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items()))
    print(f"fuzz_bck {fam} seed={seed}" + (f" tile={tile}" if tile else "") + f": {total} cases, {bad} mismatches; worst fraction of each float64 bound: {worst}; "
          "kernels / tile configs used:", dict(sorted(T.USED.items(), key=lambda kv: -kv[1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
