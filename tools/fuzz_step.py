#!/usr/bin/env python3
"""Seeded random-geometry sweeps for the functions of a training step that are not convolutions: the training BatchNorm (kernels/bn_f32.hip: the hip_bn_*, hip_bnc_*
and hip_bnf_* families), the full SoftmaxWithLoss (kernels/loss_f32.hip), the solver family (kernels/sgd_update_f32.hip, solver_update_f32.hip), the evaluation functions (kernels/eval_f32.hip)
and hip_data_transform (kernels/data_f32.hip).

usage: fuzz_step.py [n_cases] [seed] [bn|bnc|bnf|loss|solver|eval|data|all]     (GPU box; run it on its own under `timeout`)
One process, one be=hip backend.  Every case runs the checks of tests/test_gpu_step_fuzz.py (the HIP kernels against be=cpu and the numpy twins of tests/bn_ref.py,
bnc_ref.py, freeze_ref.py, loss_ref.py, sgd_ref.py, solver_ref.py, accum_ref.py, eval_ref.py and data_ref.py by bits; prob and loss_per_pel under loss_ref's written bounds).  A failed compare prints `MISMATCH <family> <case> <what>`,
the last line is the summary (cases, mismatches, the worst fraction of each bound, the kernels used) and the exit code is 1 on any mismatch.  Anything that is not a
failed compare -- an HIP error included -- ends the run at once.

The case generators and the category functions below are importable without a GPU (nothing here touches torch, HIP or a backend at import) and are pure functions of
(n, seed) on np.random.default_rng; tests/test_step_fuzz_cpu.py checks them and runs every check on be=cpu on the very cases the GPU test uses.  The category functions
restate, in Python, which branch of a kernel a geometry reaches: bn_slab_plan (csrc/rtc_types.h) and the walk of bodahip_bn_sum, plan_loss_op (csrc/native_plan.cc) and
the thread numbering of the three loss kernels.  They do not call the planner."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np

ELEM_CAP = 200000   # elements per tensor: the numpy twins loop per round of a chain
F = np.float32


def _cdiv(a, b):
    return -(-a // b)


# ---- the training BatchNorm: case = ((B, C, H, W), forced slab, data kind)
BN_KINDS = ("normal", "offset", "flat")
BN_FORCED = (0, 0, 0, 4, 8, 48, 100, 1024, 2000, 2048, 5000)
BN_CHANS = (1, 2, 3, 5, 8)
BN_MAX_SLABS = 4096


def bn_slab_plan(C, N, forced=0):
    """bn_slab_plan (csrc/rtc_types.h), restated -> (slab, nslabs): 512 workgroups wanted, a planned slab a multiple of 1024 and at least 4096."""
    if forced:
        slab = forced
    else:
        want = max(1, _cdiv(512, C))
        slab = max(_cdiv(_cdiv(N, want), 1024) * 1024, 4096)
    return slab, max(1, _cdiv(N, slab))


def bn_slab_lens(C, N, forced=0):
    slab, ns = bn_slab_plan(C, N, forced)
    return [min(slab, N - s * slab) for s in range(ns)]


def bn_categories(case):
    """The branches of bodahip_bn_sum (and of the finalising kernel) a case reaches, by name.  A slab of len elements has ceil(len / 4) quads; thread t takes quads t,
    t + 256, ...; the host gives the kernel (step_img, step_pel) = (1024 / HW, 1024 % HW), the walk from one of a chain's quads to its next.
    quad path (HW % 4 == 0)   q_gt1024 (a slab of more than 1024 elements: the walk is taken, a load with k >= 1 in flight), q_gt4096 (the outer round q += 1024), and on
                              a slab of more than 1024 elements q_step_pel0 (1024 % HW == 0, HW < 1024), q_carry (1024 % HW != 0, HW < 1024: the single carry),
                              q_step_img0 (HW > 1024), q_hw1024
    element path              e_hw1, e_hw2, e_hw3 (N >= 64: a quad across three or four images, the while carry), e_odd_gt1024 (HW odd and above 1024), e_edge_in_plane
                              (two or more slabs and slab % HW != 0), e_gt1024 (a slab of more than 1024 elements)
    either                    ragged_last (two or more slabs, the last no multiple of 1024), empty_chains (a slab of fewer than 1021 elements: a chain without one),
                              planner3 (the planner's own plan with three or more slabs), slabs2 (two or more slabs), c1 / c255 / c256 / c257, n1, and the data kind"""
    (B, C, H, W), forced, kind = case
    HW = H * W
    N = B * HW
    slab, ns = bn_slab_plan(C, N, forced)
    lens = bn_slab_lens(C, N, forced)
    cats = {"quad" if HW % 4 == 0 else "elem", kind}
    if HW % 4 == 0:
        if max(lens) > 1024:
            cats.add("q_gt1024")
            cats.add("q_hw1024" if HW == 1024 else "q_step_img0" if HW > 1024 else "q_step_pel0" if 1024 % HW == 0 else "q_carry")
        if max(lens) > 4096: cats.add("q_gt4096")
    else:
        if HW <= 3 and N >= 64: cats.add(f"e_hw{HW}")
        if HW % 2 and HW > 1024: cats.add("e_odd_gt1024")
        if ns >= 2 and slab % HW: cats.add("e_edge_in_plane")
        if max(lens) > 1024: cats.add("e_gt1024")
    if ns >= 2:
        cats.add("slabs2")
        if lens[-1] % 1024: cats.add("ragged_last")
    if min(lens) < 1021: cats.add("empty_chains")
    if not forced and ns >= 3: cats.add("planner3")
    if C in (1, 255, 256, 257): cats.add(f"c{C}")
    if N == 1: cats.add("n1")
    return cats


BN_WANTS = {
    "quad": ["q_gt1024", "q_gt4096", "q_step_pel0", "q_carry", "q_step_img0", "q_hw1024", "ragged_last", "empty_chains", "planner3"],
    "elem": ["e_hw1", "e_hw2", "e_hw3", "e_odd_gt1024", "e_edge_in_plane", "c1", "c255", "c256", "c257", "n1", "planner3"],
}


def _bn_draw(rng, want, path):
    B, C = int(rng.integers(1, 7)), int(rng.choice(BN_CHANS))
    H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    forced = int(rng.choice(BN_FORCED))
    kind = BN_KINDS[int(rng.choice([0, 0, 0, 1, 2]))]
    if path == "quad":
        W = 4 * int(rng.integers(1, 11))
    if want == "q_gt1024":
        forced = int(rng.choice([0, 2000, 2048]))
    elif want == "q_gt4096":
        forced = int(rng.choice([0, 5000])); B = int(rng.integers(3, 7)); H = int(rng.integers(20, 41))
    elif want == "q_step_pel0":
        H, W = (int(v) for v in rng.choice([(1, 4), (2, 4), (4, 4), (4, 8), (8, 8), (8, 16), (16, 16), (16, 32)])); B = int(rng.integers(_cdiv(1100, H * W), _cdiv(9000, H * W) + 1)); forced = int(rng.choice([0, 2000, 2048, 5000]))
    elif want == "q_carry":
        forced = int(rng.choice([0, 2000, 2048, 5000])); H = int(rng.integers(1, 25))
    elif want == "q_step_img0":
        H = int(rng.integers(33, 41)); W = int(rng.choice([32, 36, 40])); forced = int(rng.choice([0, 2000, 2048, 5000]))
    elif want == "q_hw1024":
        H, W = (32, 32) if rng.random() < 0.5 else (64, 16); B = int(rng.integers(2, 7)); forced = int(rng.choice([0, 2000, 2048, 5000]))
    elif want == "ragged_last":
        forced = int(rng.choice([100, 1024, 2000, 2048, 5000]))
    elif want == "planner3":
        C = int(rng.choice([1, 2, 3])); forced = 0
        if path == "quad":
            H, W = int(rng.integers(30, 41)), int(rng.choice([32, 36, 40])); B = int(rng.integers(_cdiv(8193, H * W), 41))
        else:
            H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41)); B = int(rng.integers(_cdiv(8193, H * W), _cdiv(8193, H * W) + 40))
    elif want in ("e_hw1", "e_hw2", "e_hw3"):
        hw = int(want[-1]); H, W = (1, hw) if rng.random() < 0.5 else (hw, 1); B = int(rng.integers(_cdiv(64, hw), 400)); forced = int(rng.choice([0, 0, 48, 100, 1024]))
    elif want == "e_odd_gt1024":
        H, W = 2 * int(rng.integers(16, 20)) + 1, 2 * int(rng.integers(16, 20)) + 1; forced = int(rng.choice([0, 2000, 2048, 5000]))
    elif want == "e_edge_in_plane":
        forced = int(rng.choice([4, 8, 48, 100, 1024, 2000]))
    elif want in ("c1", "c255", "c256", "c257"):
        C = int(want[1:]); H, W = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    elif want == "n1":
        B = H = W = 1
    return ((B, C, H, W), forced, kind)


def bn_cases(n, seed, path):
    """n BatchNorm cases ((B, C, H, W), forced slab, kind) for the load path `path` ("quad": W a multiple of 4 | "elem": any plane).  B 1-6 (more where a category needs
    a long channel); C from BN_CHANS or 255 / 256 / 257; planes 1-40 a side (64 x 16 among the planes of 1024 pels); the forced slab from BN_FORCED (0: the planner's); the data kind from BN_KINDS, three in five
    `normal`.  A draw is rejected where a tensor has more than ELEM_CAP elements or the forced slab cuts a channel into more than 4096 slabs (the op is refused).  Seven of
    every eight cases are bent towards one of BN_WANTS[path] in turn (drawn again until the category holds on the path)."""
    rng = np.random.default_rng(seed)
    wants = BN_WANTS[path]
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else wants[(i - i // 8) % len(wants)]
        for _ in range(4000):
            case = _bn_draw(rng, want, path)
            (B, C, H, W), forced, kind = case
            if B * C * H * W > ELEM_CAP or bn_slab_plan(C, B * H * W, forced)[1] > BN_MAX_SLABS:
                continue
            cats = bn_categories(case)
            if (path == "quad") != ("quad" in cats) and not (path == "elem" and want in ("c1", "c255", "c256", "c257", None)):
                continue
            if want is None or want in cats:
                break
        else:
            raise RuntimeError(f"bn_cases: no draw reached category {want} of {path}")
        out.append(case)
    return out


def bn_inputs(case, seed):
    """bn_ref.make_inputs' dict for a case.  normal: make_inputs itself.  offset: x = 1e3 + 1e-2 N(0, 1), so that a one-pass variance would cancel.  flat: x = 1e-20
    N(0, 1): every square underflows, var is 0 and inv_std = 1 / sqrt(eps).  (No constant channel in the last two: the kind is the point.)"""
    import bn_ref
    shape, _, kind = case
    i = bn_ref.make_inputs(shape, seed)
    if kind != "normal":
        g = np.random.default_rng([seed, 78, *shape]).standard_normal(shape)
        i["x"] = (1e3 + 1e-2 * g).astype(F) if kind == "offset" else (1e-20 * g).astype(F)
    return i


# ---- the chunked chain: case = ((B, C, H, W), chunks, forced slab, kind)
BNC_WANTS = ["empty_chunk", "chunk_of_one", "ragged_chunks", "chunk_slabs2"]


def bnc_chunks(B, n):
    return [(B * i // n, B * (i + 1) // n) for i in range(n)]


def bnc_categories(case):
    """empty_chunk (chunks > B), chunk_of_one (a chunk of one image), ragged_chunks (chunks <= B does not divide B), chunk_slabs2 (a chunk whose own plan has two or more
    slabs), and bn_categories of the largest chunk's own dims with a `chunk_` in front."""
    (B, C, H, W), n, forced, kind = case
    sizes = [b1 - b0 for b0, b1 in bnc_chunks(B, n)]
    cats = set()
    if n > B: cats.add("empty_chunk")
    if 1 in sizes: cats.add("chunk_of_one")
    if n <= B and B % n: cats.add("ragged_chunks")
    if any(s and bn_slab_plan(C, s * H * W, forced)[1] >= 2 for s in sizes): cats.add("chunk_slabs2")
    cats |= {"chunk_" + c for c in bn_categories(((max(sizes), C, H, W), forced, kind))}
    return cats


def bnc_cases(n, seed):
    """n chunked cases: the geometry draws of bn_cases (both paths by turns, unbent or bent towards a long channel), chunks from {2, 3, 5, B, B + 1}; seven of every eight
    bent towards one of BNC_WANTS in turn."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else BNC_WANTS[(i - i // 8) % len(BNC_WANTS)]
        path = ("quad", "elem")[i % 2]
        for _ in range(4000):
            geo = _bn_draw(rng, ("q_gt1024" if path == "quad" else "e_edge_in_plane") if want == "chunk_slabs2" else None, path)
            (B, C, H, W), forced, kind = geo
            if want == "chunk_slabs2" and not forced:
                forced = 2000
            ch = int(rng.choice([2, 3, 5, B, B + 1]))
            case = ((B, C, H, W), ch, forced, kind)
            if B * C * H * W > ELEM_CAP or bn_slab_plan(C, H * W, forced)[1] * B > BN_MAX_SLABS or ((H * W) % 4 == 0) != (path == "quad"):
                continue
            if want is None or want in bnc_categories(case):
                break
        else:
            raise RuntimeError(f"bnc_cases: no draw reached category {want}")
        out.append(case)
    return out


# ---- SoftmaxWithLoss: case = ((B, C, H, W), label seed, label set, normalisation, weight, logits kind)
LOSS_NORMS = ("valid", "full", "batch_size", "none")
LOSS_WEIGHTS = (1.0, 0.3, 0.0)
LOSS_DATA = ("pm4", "wide", "low")
LOSS_SETS = ("valid", "ign255", "ign0", "ign-1", "all_ignored", "invalid_C", "invalid_nan")   # loss_ref.label_sets' names, in its order
LOSS_CREG = 32


def loss_form(shape):
    """plan_loss_op's rule: the pel form from 64 pels a plane on."""
    return "pel" if shape[2] * shape[3] >= 64 else "wave"


def loss_plan(shape):
    """plan_loss_op (csrc/native_plan.cc), restated -> {function: (grid, the forward's CREG)}; 256 threads a workgroup."""
    B, C, H, W = shape
    pels = B * H * W
    pel = loss_form(shape) == "pel"
    return {"fwd": (_cdiv(pels if pel else pels * 64, 256), C if pel and C <= LOSS_CREG else 0), "norm": (1, 0), "bck": (_cdiv(_cdiv(pels * C, 4), 256), 0)}


def loss_categories(case):
    """hw63 / hw64 / hw65 (the form switch); pel form: pel_c1, pel_c31, pel_c32, pel_c33, pel_c_gt64 (CREG = C up to 32, the re-reading form above); wave form: wave_c_lt64
    (lanes without a channel), wave_c64, wave_c_65_127 (a ragged second round), wave_c_ge192_ragged; n_lt256, n_eq256, n_gt256_ragged (bodahip_loss_norm's chains: B * HW
    against 256); e_not_quad (B * C * HW % 4 != 0: the gradient's scalar tail); tiny_plane (HW < 4 and C * HW < 4: one quad of the gradient across images); all_ignored;
    ignore_in_range (an ignore_label in [0, C)); fwd_ragged_wg (the forward's last workgroup partly filled)."""
    shape, lseed, lset, nz, w, kind = case
    B, C, H, W = shape
    HW = H * W
    n = B * HW
    cats = {loss_form(shape), kind, nz, LOSS_SETS[lset]}
    if HW in (63, 64, 65): cats.add(f"hw{HW}")
    if loss_form(shape) == "pel":
        if C in (1, 31, 32, 33): cats.add(f"pel_c{C}")
        if C > 64: cats.add("pel_c_gt64")
        if n % 256: cats.add("fwd_ragged_wg")
    else:
        if C < 64: cats.add("wave_c_lt64")
        if C == 64: cats.add("wave_c64")
        if 64 < C < 128: cats.add("wave_c_65_127")
        if C >= 192 and C % 64: cats.add("wave_c_ge192_ragged")
        if n % 4: cats.add("fwd_ragged_wg")
    cats.add("n_lt256" if n < 256 else "n_eq256" if n == 256 else "n_gt256_ragged" if n % 256 else "n_whole_rounds")
    if (n * C) % 4: cats.add("e_not_quad")
    if HW < 4 and C * HW < 4: cats.add("tiny_plane")
    if LOSS_SETS[lset] == "ign0": cats.add("ignore_in_range")
    return cats


LOSS_WANTS = {
    "pel": ["hw64", "hw65", "pel_c1", "pel_c31", "pel_c32", "pel_c33", "pel_c_gt64", "n_eq256", "n_gt256_ragged", "e_not_quad", "all_ignored"],
    "wave": ["hw63", "wave_c_lt64", "wave_c64", "wave_c_65_127", "wave_c_ge192_ragged", "n_lt256", "tiny_plane", "ignore_in_range", "e_not_quad", "n_eq256", "all_ignored"],
}


def _loss_draw(rng, want, form):
    B = int(rng.integers(1, 6))
    C = int(rng.choice([1, 2, 3, 5, 21, 31, 32, 33, 63, 64, 65, 70, 100, 127, 128, 200, 257, 1000]))
    if form == "pel":
        H, W = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        if H * W < 64:
            H, W = int(rng.integers(8, 25)), int(rng.integers(8, 25))
    else:
        H = int(rng.integers(1, 8)); W = int(rng.integers(1, _cdiv(64, H) + 1))
    lset = int(rng.integers(0, len(LOSS_SETS)))
    if want in ("hw63", "hw64", "hw65"):
        hw = int(want[2:]); H, W = [(a, hw // a) for a in range(1, hw + 1) if hw % a == 0][int(rng.integers(0, 3 if hw != 64 else 7))]
    elif want and want.startswith("pel_c"):
        C = int(rng.choice([65, 70, 100, 129])) if want == "pel_c_gt64" else int(want[5:])
    elif want == "wave_c_lt64":
        C = int(rng.integers(1, 64))
    elif want == "wave_c64":
        C = 64
    elif want == "wave_c_65_127":
        C = int(rng.integers(65, 128))
    elif want == "wave_c_ge192_ragged":
        C = int(rng.choice([193, 200, 257, 1000]))
    elif want == "n_eq256":
        B, H, W = [(1, 16, 16), (4, 8, 8), (2, 8, 16), (4, 64, 1)][int(rng.integers(0, 4))] if form == "pel" else [(4, 8, 8), (16, 4, 4), (256, 1, 1), (8, 4, 8), (64, 2, 2)][int(rng.integers(1, 5))]
    elif want == "n_gt256_ragged" and form == "wave":
        B = int(rng.integers(40, 90))
    elif want == "tiny_plane":
        H, W = 1, int(rng.integers(1, 4)); C = int(rng.integers(1, _cdiv(4, W))); B = int(rng.integers(2, 40))
    elif want == "all_ignored":
        lset = LOSS_SETS.index("all_ignored")
    elif want == "ignore_in_range":
        lset = LOSS_SETS.index("ign0")
    w = float(rng.choice(LOSS_WEIGHTS)) if rng.random() < 0.5 else float(F(rng.uniform(0.01, 4.0)))
    return ((B, C, H, W), int(rng.integers(0, 1 << 16)), lset, str(rng.choice(LOSS_NORMS)), w, str(rng.choice(LOSS_DATA)))


def loss_cases(n, seed, form):
    """n loss cases ((B, C, H, W), label seed, index into loss_ref.label_sets, normalisation, weight, logits kind) for the forward's form `form` ("pel" | "wave").  B 1-5
    (more where a category needs pels); C from 1 to 1000 around the 32 / 64 edges; planes up to 24 x 24 (pel) or below 64 pels (wave); the weight one of loss_ref.WEIGHTS or
    drawn in (0, 4).  Seven of every eight cases are bent towards one of LOSS_WANTS[form] in turn."""
    rng = np.random.default_rng(seed)
    wants = LOSS_WANTS[form]
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else wants[(i - i // 8) % len(wants)]
        for _ in range(4000):
            case = _loss_draw(rng, want, form)
            B, C, H, W = case[0]
            if B * C * H * W > ELEM_CAP or loss_form(case[0]) != form:
                continue
            if want is None or want in loss_categories(case):
                break
        else:
            raise RuntimeError(f"loss_cases: no draw reached category {want} of {form}")
        out.append(case)
    return out


# ---- the solver family: an update case = (sizes, lr_mults, decay_mults, (lr, momentum, weight_decay, momentum2, delta, t), coef)
SOLVER_SIZES = (1, 2, 3, 4, 5, 255, 1023, 4095, 4096, 4097, 8191, 8192, 8193)
SOLVER_MULTS = (0.0, 0.5, 1.0, 2.0)
SOLVER_CHUNK = 4096
SOLVER_WANTS = ["t1", "t31", "t32", "one_chunk", "chunk_plus", "lt4", "all_ragged"]


def solver_grid(sizes):
    """One workgroup per chunk of 4096 floats, chunks numbered over the tensors in order (the update, hip_grad_sumsq and hip_grad_accum alike)."""
    return sum(_cdiv(n, SOLVER_CHUNK) for n in sizes)


def solver_categories(case):
    """t1 / t31 / t32 (tens_num), one_chunk (a tensor of exactly 4096), chunk_plus (one chunk and 1 to 3 scalars), lt4 (a tensor below one quad), all_ragged (no size a
    multiple of 4), drawn_size (a size outside SOLVER_SIZES)."""
    sizes = case[0]
    cats = set()
    if len(sizes) in (1, 31, 32): cats.add(f"t{len(sizes)}")
    if 4096 in sizes: cats.add("one_chunk")
    if any(4096 < n < 4100 for n in sizes): cats.add("chunk_plus")
    if any(n < 4 for n in sizes): cats.add("lt4")
    if all(n % 4 for n in sizes): cats.add("all_ragged")
    if any(n not in SOLVER_SIZES for n in sizes): cats.add("drawn_size")
    return cats


def _solver_draw(rng, want):
    T = int(rng.integers(1, 33))
    if want in ("t1", "t31", "t32"):
        T = int(want[1:])
    pool = [n for n in SOLVER_SIZES if n % 4] if want == "all_ragged" else list(SOLVER_SIZES)
    sizes = [int(rng.choice(pool)) if rng.random() < 0.8 else int(rng.integers(1, 20001)) for _ in range(T)]
    if want == "one_chunk": sizes[int(rng.integers(0, T))] = 4096
    if want == "chunk_plus": sizes[int(rng.integers(0, T))] = 4096 + int(rng.integers(1, 4))
    if want == "lt4": sizes[int(rng.integers(0, T))] = int(rng.integers(1, 4))
    lm = tuple(float(rng.choice(SOLVER_MULTS)) for _ in range(T)); dm = tuple(float(rng.choice(SOLVER_MULTS)) for _ in range(T))
    hy = (float(F(rng.uniform(1e-3, 0.5))), float(rng.choice([0.0, 0.25, 0.9])), float(rng.choice([0.0, 5e-4, 0.125])), float(rng.choice([0.5, 0.9, 0.999])),
          float(rng.choice([1e-8, 1e-3])), int(rng.integers(1, 4)))
    return (tuple(sizes), lm, dm, hy, float(F(rng.uniform(0.05, 1.5))))


def solver_cases(n, seed):
    """n update cases: tens_num 1-32; sizes from SOLVER_SIZES, one in five drawn in 1-20000; lr_mult / decay_mult from SOLVER_MULTS per tensor; hyper-parameters
    from the ranges tests/solver_ref.py uses; the clipping coefficient in (0.05, 1.5).  Seven of every eight bent towards one of SOLVER_WANTS in turn."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else SOLVER_WANTS[(i - i // 8) % len(SOLVER_WANTS)]
        for _ in range(4000):
            case = _solver_draw(rng, want)
            if sum(case[0]) <= ELEM_CAP and (want is None or want in solver_categories(case)):
                break
        else:
            raise RuntimeError(f"solver_cases: no draw reached category {want}")
        out.append(case)
    return out


# the norm: case = ([(part0, sizes)] the hip_grad_sumsq calls, parts_total, clip kind)
NORM_CLIPS = ("below", "above", "equal", "off")


def norm_categories(case):
    calls, total, clip = case
    cats = {"clip_" + clip}
    if total > 256: cats.add("parts_gt256")
    if total > 512: cats.add("parts_gt512")
    if len(calls) > 1: cats.add("calls2")
    if any(n > SOLVER_CHUNK for _, sz in calls for n in sz): cats.add("tensor_chunks2")
    return cats


def norm_cases(n, seed):
    """n norm cases.  Every fourth has about 300 tensors of 1 to 5 elements, at most 32 a call, so that hip_grad_norm sees more than 256 partials (the second round of
    its lanes); the others 1-40 tensors from SOLVER_SIZES.  The calls own rising ranges of one partials var, with 0-2 slots nobody owns in front and behind; the clip
    kind goes round NORM_CLIPS (below / above / equal to the norm the twin gives; off = 0)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 4 == 1:
            sizes = [int(v) for v in rng.integers(1, 6, int(rng.integers(290, 330)))]
        else:
            sizes = [int(rng.choice(SOLVER_SIZES)) for _ in range(int(rng.integers(1, 41)))]
        p0 = int(rng.integers(0, 3)); calls = []
        while sizes:
            k = int(rng.integers(1, 33)) if i % 4 != 1 else 32
            calls.append((p0, tuple(sizes[:k]))); p0 += solver_grid(sizes[:k]); sizes = sizes[k:]
        out.append((tuple(calls), p0 + int(rng.integers(0, 3)), NORM_CLIPS[i % 4 if i % 8 < 4 else (i + 1) % 4]))
    return out


# ---- the evaluation functions (kernels/eval_f32.hip)
ACC_VALUES = (-2.0, -0.5, -0.0, 0.0, 0.25, 1.0, 1.0, 3.5)   # the eight logit values: ties are the rule, +0 against -0 among them
ACC_BAD_LABELS = (-1.0, None, float("nan"), 1e9)              # (None: the label C)
ACC_WANTS = ["ragged_both", "c_gt64", "c_lt64", "b1", "c1", "whole_wg"]
ACCUM_WANTS = ["b_255_257", "b_511_513", "k1", "k2", "kC", "kC3"]


def eval_grids(kind, B=0, C=0):
    """plan_eval_op (csrc/native_plan.cc), restated: hip_accuracy one wave an image, four a workgroup; hip_eval_accum one workgroup; hip_bn_fold one thread a channel."""
    return {"accuracy": _cdiv(B, 4), "accum": 1, "fold": _cdiv(C, 256)}[kind]


def acc_categories(case):
    """hip_accuracy, case = (B, C, invalid share, seed): ragged_both (B % 4 and C % 64 both non-zero), c_gt64 (a lane with two or more channels), c_lt64 (lanes without a
    channel), b1, c1, whole_wg (B % 4 == 0), invalid (a share of invalid labels)."""
    B, C, share, seed = case
    cats = set()
    if B % 4 and C % 64: cats.add("ragged_both")
    if C > 64: cats.add("c_gt64")
    if C < 64: cats.add("c_lt64")
    if B == 1: cats.add("b1")
    if C == 1: cats.add("c1")
    if B % 4 == 0: cats.add("whole_wg")
    if share > 0: cats.add("invalid")
    return cats


def acc_cases(n, seed):
    """n hip_accuracy cases (B, C, share of invalid labels, data seed): B 1-40 and C 1-1100 drawn together; seven of every eight bent towards one of ACC_WANTS in turn."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else ACC_WANTS[(i - i // 8) % len(ACC_WANTS)]
        for _ in range(4000):
            B, C = int(rng.integers(1, 41)), int(rng.integers(1, 1101)) if rng.random() < 0.6 else int(rng.integers(1, 130))
            if want == "b1": B = 1
            if want == "c1": C = 1
            if want == "c_lt64": C = int(rng.integers(1, 64))
            case = (B, C, float(rng.choice([0.0, 0.1, 0.3, 1.0])), int(rng.integers(0, 1 << 16)))
            if want is None or want in acc_categories(case):
                break
        out.append(case)
    return out


def acc_data(case):
    """-> (x float (B, C, 1, 1) drawn from ACC_VALUES, label float (B, 1, 1): a class, or with the case's share one of -1, C, NaN, 1e9)."""
    B, C, share, seed = case
    rng = np.random.default_rng([seed, 61])
    x = np.array(ACC_VALUES, F)[rng.integers(0, len(ACC_VALUES), (B, C))].reshape(B, C, 1, 1)
    lab = rng.integers(0, C, B).astype(F)
    for i in np.nonzero(rng.random(B) < share)[0]:
        v = ACC_BAD_LABELS[int(rng.integers(0, len(ACC_BAD_LABELS)))]
        lab[i] = F(C) if v is None else F(v)
    return x, lab.reshape(B, 1, 1)


def accum_categories(case):
    """hip_eval_accum, case = (B, C, top_k, seed): b_255_257 / b_511_513 (around one and two rounds of the 256 lanes), k1 / k2 / kC / kC3 (top_k = 1, 2, C, C + 3)."""
    B, C, top_k, seed = case
    cats = set()
    if 255 <= B <= 257: cats.add("b_255_257")
    if 511 <= B <= 513: cats.add("b_511_513")
    for k, nm in ((1, "k1"), (2, "k2"), (C, "kC"), (C + 3, "kC3")):
        if top_k == k: cats.add(nm)
    return cats


def accum_cases(n, seed):
    """n hip_eval_accum cases (B, C, top_k, data seed): B from 255-257 and 511-513 or drawn in 1-700, C 3-20, top_k from {1, 2, C, C + 3}."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else ACCUM_WANTS[(i - i // 8) % len(ACCUM_WANTS)]
        for _ in range(4000):
            C = int(rng.integers(3, 21))
            B = int(rng.choice([255, 256, 257, 511, 512, 513])) if rng.random() < 0.7 else int(rng.integers(1, 701))
            case = (B, C, int(rng.choice([1, 2, C, C + 3])), int(rng.integers(0, 1 << 16)))
            if want is None or want in accum_categories(case):
                break
        out.append(case)
    return out


def fold_cases(n, seed):
    """n hip_bn_fold cases (C, eval_ref.fold_inputs' seed): C 1-600, by turns below, at and above the workgroups' edges 256 and 512 and drawn."""
    rng = np.random.default_rng(seed)
    edges = (1, 255, 256, 257, 511, 512, 513)
    return [(int(edges[i // 2 % len(edges)]) if i % 2 == 0 else int(rng.integers(1, 601)), int(rng.integers(0, 1 << 16))) for i in range(n)]


# ---- hip_data_transform: case = tests/data_ref.py's dict (chan, cw, ch, dw, dh, B, layout, pel, scale, k) with a plan seed `ps`
DATA_SCALES = (1.0, 1.0 / 256, 0.017, -1.0, 0.0)
DATA_WANTS = ["cw1", "cw2", "cw3", "not_quad", "crop_is_src", "hwc", "chw", "pel_mean"]
DATA_MIRRORS = (0, 1, 0xFFFFFFFF)
DATA_STEPS = 3


def data_grid(c):
    """plan_data_op, restated: a thread owns four flat output elements."""
    return _cdiv(_cdiv(c["B"] * c["chan"] * c["ch"] * c["cw"], 4), 256)


def data_plans(c):
    """-> DATA_STEPS uint32 (B, 4) plans: per image offsets drawn from {0, half the range, the range (at the clamp), the range + 1, 2^20, 0xFFFFFFFF (beyond it)}, the
    mirror word from DATA_MIRRORS, word 3 garbage; image 0 of the first step mirrors with an x offset beyond the clamp."""
    rng = np.random.default_rng([c["ps"], 71])
    plans = []
    for s in range(DATA_STEPS):
        rows = []
        for i in range(c["B"]):
            oy = [0, c["dh"] // 2, c["dh"], c["dh"] + 1, 1 << 20, 0xFFFFFFFF][int(rng.integers(0, 6))]
            ox = [0, c["dw"] // 2, c["dw"], c["dw"] + 1, 1 << 20, 0xFFFFFFFF][int(rng.integers(0, 6))]
            rows.append((oy, ox, DATA_MIRRORS[int(rng.integers(0, 3))], 0xA5A5F00D ^ (s * 16 + i)))
        if s == 0:
            rows[0] = (rows[0][0], c["dw"] + 1 + int(rng.integers(0, 2)) * 0xFFFF, int(rng.choice(DATA_MIRRORS[1:])), rows[0][3])
        plans.append(np.array(rows, np.uint32))
    return plans


def data_categories(c):
    """cw1 / cw2 / cw3 (a thread's four elements across rows, planes and images), not_quad (ch * cw * C * B no multiple of 4), crop_is_src, hwc / chw, pel_mean /
    chan_mean, mirror_clamped (a mirrored image whose x offset is beyond the clamp), wgs2 (more than one workgroup)."""
    cats = {c["layout"], "pel_mean" if c["pel"] else "chan_mean"}
    if c["cw"] <= 3: cats.add(f"cw{c['cw']}")
    if (c["ch"] * c["cw"] * c["chan"] * c["B"]) % 4: cats.add("not_quad")
    if c["dh"] == 0 and c["dw"] == 0: cats.add("crop_is_src")
    if any(int(r[1]) > c["dw"] and int(r[2]) for p in data_plans(c) for r in p): cats.add("mirror_clamped")
    if data_grid(c) > 1: cats.add("wgs2")
    return cats


def data_cases(n, seed):
    """n hip_data_transform cases: source H, W 1-40, crop ch <= H and cw <= W, C from {1, 3, 4}, B 1-5, interleaved or planar source, per-channel or per-pel mean, the
    scale from DATA_SCALES; seven of every eight bent towards one of DATA_WANTS in turn.  `k` (data_ref.case_data's stream) is the case's index."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        i = len(out)
        want = None if i % 8 == 7 else DATA_WANTS[(i - i // 8) % len(DATA_WANTS)]
        for _ in range(4000):
            H, W = int(rng.integers(1, 41)), int(rng.integers(1, 41))
            ch, cw = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
            if want in ("cw1", "cw2", "cw3"):
                cw = int(want[2]); W = max(W, cw)
            if want == "crop_is_src":
                ch, cw = H, W
            c = dict(chan=int(rng.choice([1, 3, 4])), cw=cw, ch=ch, dw=W - cw, dh=H - ch, B=int(rng.integers(1, 6)), layout=str(rng.choice(["hwc", "chw"])),
                     pel=int(rng.integers(0, 2)), scale=float(rng.choice(DATA_SCALES)), k=i, ps=int(rng.integers(0, 1 << 16)))
            if want is None or want in data_categories(c):
                break
        out.append(c)
    return out


FAMILIES = ("bn", "bnc", "bnf", "loss", "solver", "eval", "data")
SEED_STEP = {"bn": 0, "bnc": 1000, "bnf": 2000, "loss": 3000, "solver": 4000, "eval": 5000, "data": 6000}   # the tool's families draw from different streams of one seed


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    fam = sys.argv[3] if len(sys.argv) > 3 else "all"
    if fam != "all" and fam not in FAMILIES:
        sys.exit(__doc__)
    import test_step_fuzz_cpu as T   # the checks themselves (tests/test_gpu_step_fuzz.py runs the same functions)
    from boda_amd.rtc import make_rtc
    hip = make_rtc("(be=hip)", 0); hip.init()
    cpu = make_rtc("(be=cpu)"); cpu.init()
    jobs = []   # (family, case, check)
    fams = FAMILIES if fam == "all" else (fam,)
    if "solver" in fams:
        s0 = seed + SEED_STEP["solver"]
        for i, case in enumerate(solver_cases(n, s0)):
            jobs.append(("solver update", case[0], lambda case=case, s=s0 + i: T.check_solver_case(hip, cpu, case, s)))
        for i, case in enumerate(norm_cases(n, s0 + 1)):
            jobs.append(("solver norm", (case[1], case[2]), lambda case=case, s=s0 + 500 + i: T.check_norm_case(hip, cpu, case, s)))
    if "eval" in fams:
        s0 = seed + SEED_STEP["eval"]
        for case in acc_cases(n, s0):
            jobs.append(("eval accuracy", case, lambda case=case: T.check_acc_case(hip, cpu, case)))
        for case in accum_cases(n, s0 + 1):
            jobs.append(("eval accum", case, lambda case=case: T.check_accum_case(hip, cpu, case)))
        for case in fold_cases(n, s0 + 2):
            jobs.append(("eval fold", case, lambda case=case: T.check_fold_case(hip, cpu, case)))
    if "data" in fams:
        for case in data_cases(n, seed + SEED_STEP["data"]):
            jobs.append(("data", {k: v for k, v in case.items() if k != "scale"}, lambda case=case: T.check_data_case(hip, cpu, case)))
    for f in [f for f in fams if f in ("bn", "bnc", "bnf", "loss")]:
        for j, path in enumerate(("quad", "elem") if f in ("bn", "bnf") else ("pel", "wave") if f == "loss" else ("",)):
            s0 = seed + SEED_STEP[f] + j
            cases = bn_cases(n, s0, path) if f in ("bn", "bnf") else loss_cases(n, s0, path) if f == "loss" else bnc_cases(n, s0)
            for i, case in enumerate(cases):
                chk = {"bn": T.check_bn_case, "bnc": T.check_bnc_case, "bnf": T.check_bnf_case, "loss": T.check_loss_case}[f]
                jobs.append((f"{f} {path}".strip(), case, lambda chk=chk, case=case, s=s0 + i: chk(hip, cpu, case, s)))
    bad = 0
    try:
        for f, case, chk in jobs:
            try:
                chk()
            except AssertionError as e:   # a failed compare; every other exception (an HIP error included) ends the run
                bad += 1
                print("MISMATCH", f, case, str(e).splitlines()[0] if str(e) else repr(e), flush=True)
    finally:
        hip.close(); cpu.close()
    worst = ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items()))
    print(f"fuzz_step {fam} seed={seed}: {len(jobs)} cases, {bad} mismatches; worst fraction of each bound: {worst}; kernels used:", dict(sorted(T.USED.items(), key=lambda kv: -kv[1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
