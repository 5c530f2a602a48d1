"""What the special-data tests of the backward kernels share (tests/test_bck_special_cpu.py, tests/test_gpu_bck_special.py): the backward twin of
tests/fwd_special_ref.py, whose pieces it imports -- seeded generators of the data classes for the three convolution gradients, their references (be=cpu and the
written chain emulators of oracle/bck_chain.py and tests/bconv_fb_ref.py, computed once and left read-only), the blindness caps, one runner for every native function
(a payload NaN in every OUT var before every run, a 4-float guard var behind every var, every IN arg read back), and the comparisons.

The contract under test is DESIGN.md section 3.11a (B1 stores, B2 finite data of any magnitude, B3 non-finite data).  Geometries are the tuples
(B, C, H, W, OC, KH, KW, SY, SX, PY, PX) of tests/test_gpu_bck_conv.EDGE.  Data classes, per gradient ("in": the data gradient, "filts": the filter gradient,
"biases": the bias gradient):
  wide            every tensor from fwd_special_ref._wide (2^-40 .. 2^30, ~5 % +0 and ~5 % -0)
  subnormal       in / filts log-uniform in 2^-76 .. 2^-62, out_grad_loss in 2^(-76+s) .. 2^(-62+s), s = SHIFT[(class, gradient, shape)]
  overflow        in / filts in 2^55 .. 2^64, out_grad_loss in 2^(55+s) .. 2^(64+s)
  nan_inf         U(-5, 5); 4 - 6 NaNs (the four patterns of NAN_BITS) and 2 - 4 +-Inf in out_grad_loss, no two of them within one window of each other in an image
  nan_inf_in      the same base; the NaNs and Infs in `in` (filter gradient)
  nan_inf_filts   the same base; one NaN and one Inf in `filts` (data gradient): the stated exception, held to containment in the injected in_chan
  bf16_saturate   the same base; finite fp32 values at or above 0x7F7F8000 in out_grad_loss (bf16_saturate_in: in `in`), which round to a bf16 Inf
The bias gradient sums out_grad_loss alone, so its `subnormal` / `overflow` windows are out_grad_loss's own: the same table moves them by about -64 / +63 binades."""
import functools

import numpy as np

import bconv_fb_ref as fb
from bconv_bf16_ref import FB_FORCED, NRMS_BOUND, U, n_terms, nrms
from boda_amd.cnn_op import OpTune, add_bck_conv_annotations, bconv_filts_biases_func_op, bf16_operands, fuse_zero_if_in_non_pos, pipe_func_args
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc
from fwd_special_ref import GUARD, NAN_BITS, POISON_BITS, _Vars, _logu, _subn, _u5, _wide, assert_no_poison, assert_same, bits, fractions, poison
from oracle import bck_chain as bc
from oracle.boda_oracle import to_bf16
from test_bck_conv_cpu import bck_op, torch_grads
from test_gpu_bck_conv import EDGE

F = np.float32
FINITE = ("wide", "subnormal", "overflow")
GRADS = ("in", "filts", "biases")
CLASSES = FINITE + ("nan_inf", "nan_inf_in", "nan_inf_filts", "bf16_saturate", "bf16_saturate_in")
SATURATE_BITS = (0x7F7F8000, 0xFF7FC000, 0x7F7FFFFF, 0xFF7F8001)     # finite fp32 values that round (to nearest even) to a bf16 Inf
T17 = (2, 17, 9, 9, 40, 3, 3, 1, 1, 1, 1)     # stride 1, two images of 81 pels (a 64-pel tile straddles them), 17 channels, K = 162 / 360
SHAPES = {n: EDGE[n] for n in ("3x3_s2_k_not_multiple_of_s", "1x1_s2_stride_gt_kernel", "5x5_s2_pad3_pad_ge_stride", "7x3_s3x2_odd_channels", "3x3_s1_img1_chan_not_32")}
SHAPES["3x3_s1_two_imgs_17_chans"] = T17
S2 = SHAPES["3x3_s2_k_not_multiple_of_s"]
# the fused filter and bias gradient's shapes: the small members of bconv_fb_ref.SHAPES (k1_long_k runs under its own forced tile only)
FB_SMALL = ("k1_ohw49_tail", "k1_ohw64_ragged", "k1_stride2", "k3_borders", "k7_stem")


def fb_shape(name):
    B, C, H, OC, k, s, p = fb.SHAPES[name]
    return (B, C, H, H, OC, k, k, s, s, p, p)


FB_SHAPES = {n: fb_shape(n) for n in FB_SMALL + ("k1_long_k",)}
FB_FORMS = [(t, n) for t, only in FB_FORCED.items() for n in (FB_SMALL if only is None else only)]

# out_grad_loss's window, moved as a whole by this many binades: per (class, gradient, shape) the move of smallest size (0, -1, +1, -2, ...) at which the REFERENCE
# (be=cpu) meets the caps below -- found on the CPU, a statement about the data alone.  The two conv gradients share out_grad_loss but have different K (OC * KH * KW
# against img * OH * OW terms); the bias gradient's sums leave the normal range only when out_grad_loss itself lies at its edge
_E = EDGE
SHIFT = {("overflow", "in", _E["1x1_s2_stride_gt_kernel"]): 1, ("overflow", "filts", _E["7x3_s3x2_odd_channels"]): 1,               # K = 36 terms each
         ("subnormal", "in", _E["3x3_s1_img1_chan_not_32"]): -1, ("overflow", "in", _E["3x3_s1_img1_chan_not_32"]): -1,               # K = 900
         ("overflow", "filts", (2, 16, 9, 9, 12, 1, 1, 2, 2, 0, 0)): 1,                                                                # K = 50
         ("subnormal", "filts", (4, 8, 28, 28, 8, 1, 1, 1, 1, 0, 0)): -2, ("overflow", "filts", (4, 8, 28, 28, 8, 1, 1, 1, 1, 0, 0)): -2,   # K = 3136
         ("subnormal", "biases", _E["3x3_s2_k_not_multiple_of_s"]): -65, ("subnormal", "biases", _E["5x5_s2_pad3_pad_ge_stride"]): -65,
         ("overflow", "biases", _E["3x3_s2_k_not_multiple_of_s"]): 62, ("overflow", "biases", T17): 62}


def shift_of(cls, grad, shape):
    return SHIFT.get((cls, grad, tuple(shape)), {"subnormal": -64, "overflow": 63}[cls] if grad == "biases" else 0)


def out_hw(shape):
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = shape
    return (H + 2 * PY - KH) // SY + 1, (W + 2 * PX - KW) // SX + 1


def sid(shape):
    return "x".join(str(v) for v in shape)


@functools.lru_cache(maxsize=None)
def op_of(shape):
    return bck_op(*shape)


def geom_of(shape):
    return op_of(tuple(shape)).bck_conv_geom()


def func_of(grad, shape, tile="", zinp=False, bf16=False):
    """The annotated function op of one gradient: "in" hip_bconv_in, "filts" hip_bconv_filts, "biases" hip_bconv_biases, "fb" hip_bconv_filts_biases."""
    op = op_of(tuple(shape))
    if grad == "fb":
        f = bconv_filts_biases_func_op(op, OpTune(hip_tile=tile))
    else:
        f = add_bck_conv_annotations(op, OpTune(hip_tile=tile))[{"in": 0, "biases": 1, "filts": 2}[grad]]
    if zinp:
        f = fuse_zero_if_in_non_pos(f)
    return bf16_operands(f) if bf16 else f


# ---------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------
def _put(arr, idx, pattern):
    bits(arr)[idx] = np.uint32(pattern)


def _apart(shape, a, b):
    """Two out pels of one image whose phase windows share no in pel: TY or more rows, or TX or more columns, apart."""
    KH, KW, SY, SX = shape[5], shape[6], shape[7], shape[8]
    return a[0] != b[0] or abs(a[1] - b[1]) >= -(-KH // SY) or abs(a[2] - b[2]) >= -(-KW // SX)


def _chan_of(kinds, n, few=False):
    """The channel of each injection, by its kind: NaNs in 0 and n // 2, +Inf in n - 1, -Inf in n // 3 -- so that a filter row / a bias holds Infs of one sign alone
    (beside a NaN an Inf does not show, and Infs of both signs in one sum are a NaN).  few: -Inf in n - 1 as well (three channels in all: of five in_chans four
    would put the filter gradient beyond the 60 % cap; its chains see the two Infs under different signs of out_grad_loss, so Infs remain)."""
    k = 0; out = []
    for kind in kinds:
        if kind == "nan":
            out.append((0, n // 2)[k % 2]); k += 1
        else:
            out.append(n - 1 if kind == "+inf" or few else n // 3)
    return out


def place_ogl(shape, rng, n_nan, n_inf):
    """-> [(img, oc, oy, ox, kind)]: the first and the last element, a border out pel, the last pel of one image and the first of the next, an interior pel, then
    random ones; a candidate within one window of an accepted one (same image) is dropped, and a small plane may end with the six directed ones (4 NaNs, 2 Infs)."""
    B, OC = shape[0], shape[4]
    OH, OW = out_hw(shape)
    cand = [(0, 0, 0), (B - 1, OH - 1, OW - 1), (0, 0, OW // 2), (0, OH - 1, OW - 1), (B - 1, 0, 0), (B - 1, OH // 2, OW // 2), (0, OH // 2, 0), (B // 2, OH - 1, 0)]
    cand += [(int(rng.integers(0, B)), int(rng.integers(0, OH)), int(rng.integers(0, OW))) for _ in range(200)]
    at = []
    for c in cand:
        if len(at) < n_nan + n_inf and all(_apart(shape, c, o) for o in at):
            at.append(c)
    assert len(at) >= 6, (shape, "no room for the injections", len(at))
    kinds = (["nan", "+inf", "nan", "-inf", "nan", "nan"] + ["nan"] * (n_nan - 4) + ["+inf", "-inf"][:n_inf - 2])[:len(at)]
    return [(img, oc, oy, ox, kind) for (img, oy, ox), oc, kind in zip(at, _chan_of(kinds, OC), kinds)]


def place_in(shape, rng, n_nan, n_inf):
    """-> [(img, c, y, x, kind)] for `in`: the same directed places on the input plane (the first pel of the last image holds a second +Inf: at a stride above the
    kernel size no term reaches the last element), then random ones."""
    B, C, H, W = shape[:4]
    at = [(0, 0, 0), (B - 1, H - 1, W - 1), (0, 0, W // 2), (0, H - 1, W - 1), (B - 1, 0, 0), (B - 1, H // 2, W // 2)]
    at = list(dict.fromkeys(at))      # (B = 1: two of the directed places coincide)
    while len(at) < n_nan + n_inf + 1:
        c = (int(rng.integers(0, B)), int(rng.integers(0, H)), int(rng.integers(0, W)))
        if c not in at:
            at.append(c)
    kinds = (["nan", "+inf", "nan", "-inf", "+inf", "nan", "nan"] + ["nan"] * (n_nan - 4) + ["+inf", "-inf"][:n_inf - 2])[:len(at)]
    return [(img, c, y, x, kind) for (img, y, x), c, kind in zip(at, _chan_of(kinds, C, few=C < 8), kinds)]


def _inject(arr, inj, saturate=False):
    n = 0
    for i, (*at, kind) in enumerate(inj):
        if saturate:
            pat = SATURATE_BITS[i % 4]; inj[i] = tuple(at) + ("+inf" if pat < 0x80000000 else "-inf",)
        elif kind == "nan":
            pat = NAN_BITS[n % 4]; n += 1
        else:
            pat = 0x7F800000 if kind == "+inf" else 0xFF800000
        _put(arr, tuple(at), pat)


def gen(cls, grad, shape, seed=0, shift=None):
    """-> {"in", "filts", "out_grad_loss", "inj": [(.., kind)], "where": the injected tensor's name}; the injected classes share their base data (`clean`)."""
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = shape
    OH, OW = out_hw(shape)
    si, sf, sg = (B, C, H, W), (OC, C, KH, KW), (B, OC, OH, OW)
    finite = cls in FINITE
    rng = np.random.default_rng([seed, FINITE.index(cls) if finite else 9, GRADS.index(grad) if finite else 0] + [int(v) for v in shape])
    sh = shift_of(cls, grad, shape) if shift is None and cls in ("subnormal", "overflow") else (shift or 0)
    d = {"inj": [], "where": None}
    if cls == "wide":
        d.update({"in": _wide(rng, si), "filts": _wide(rng, sf), "out_grad_loss": _wide(rng, sg)})
    elif cls == "subnormal":
        d.update({"in": _subn(rng, si), "filts": _subn(rng, sf, few=False), "out_grad_loss": _subn(rng, sg, shift=sh)})
    elif cls == "overflow":
        d.update({"in": _logu(rng, si, 55, 64), "filts": _logu(rng, sf, 55, 64), "out_grad_loss": _logu(rng, sg, 55 + sh, min(64 + sh, 127.99))})
    else:
        d.update({"in": _u5(rng, si), "filts": _u5(rng, sf), "out_grad_loss": _u5(rng, sg)})
        n_nan, n_inf = 4 + int(rng.integers(0, 3)), 2 + int(rng.integers(0, 3))
        if cls in ("nan_inf", "bf16_saturate"):
            d["inj"], d["where"] = place_ogl(shape, rng, n_nan, n_inf), "out_grad_loss"
        elif cls in ("nan_inf_in", "bf16_saturate_in"):
            d["inj"], d["where"] = place_in(shape, rng, n_nan, n_inf), "in"
        elif cls == "nan_inf_filts":     # a corner tap of the first in_chan, a middle tap of the last
            d["inj"], d["where"] = [(0, 0, 0, 0, "nan"), (OC - 1, C - 1, KH // 2, KW // 2, "+inf")], "filts"
        elif cls != "clean":
            raise ValueError(cls)
        if d["inj"]:
            _inject(d[d["where"]], d["inj"], saturate=cls.startswith("bf16_saturate"))
    return d


def zinp_in(shape, seed=0):
    """The forward input of the zero_if_in_non_pos form: U(-5, 5) with +0, -0, NaNs of either sign, -Inf and the smallest denormals of its own."""
    rng = np.random.default_rng([seed, 77] + [int(v) for v in shape])
    x = _u5(rng, shape[:4])
    u = rng.uniform(0, 1, x.shape)
    for lo, pat in ((0.00, 0x00000000), (0.05, 0x80000000), (0.10, 0x7FC00000), (0.13, 0xFFC00001), (0.16, 0xFF800000), (0.18, 0x00000001), (0.20, 0x80000001)):
        bits(x)[(u >= lo) & (u < lo + 0.02)] = np.uint32(pat)
    return x


# ---------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------
def run_fop(rtc, fop, datasets, pfx="bsp_", seed=None, before=()):
    """Compile one annotated function once, create its vars once (a 4-float guard var behind every var; `before`: args that get one in front as well), then for every
    data set {name: {arg: array}}: upload the IN args -- and an OUT arg the set names (an in-place function; the untouched part of a concat's output) --, refill every
    other OUT var with the payload NaN, run.  -> {name: {OUT arg: array, "launch": last_launch()}}.  Asserted here, for every run: every guard var keeps its bits,
    every IN arg reads back bit for bit."""
    spec = pipe_func_args(fop)
    fn = pfx + "f"
    vs = _Vars(rtc, pfx)
    res = {}
    try:
        rtc.compile([RtcFuncInfo(fn, "", [a for a, _ in spec], fop)])
        am = {}
        for an, io in spec:
            if io == "REF":
                am[an] = RtcArg.ref(fop.get_dims(an))
            elif io == "VAL":
                am[an] = RtcArg.scalar(seed, "uint32_t")
            else:
                if an in before:     # (created first, so that it stands in front of the var where the allocator places them in order)
                    rtc.create_var_with_dims(vs.pfx + an + "_pre_guard", Dims.make("float", v=4)); vs.made.append(vs.pfx + an + "_pre_guard")
                    rtc.copy_nda_to_var(vs.pfx + an + "_pre_guard", GUARD.view(F))
                am[an] = RtcArg.var(vs.make(an, fop.get_dims(an)))
        for name, d in datasets.items():
            for an, io in spec:
                if io in ("REF", "VAL"):
                    continue
                dims = fop.get_dims(an)
                if an in d:
                    a = np.ascontiguousarray(d[an]); a = a if a.dtype == np.uint32 and dims.tn == "uint32_t" else np.ascontiguousarray(a, F)
                    rtc.copy_nda_to_var(vs.pfx + an, a.reshape(dims.sizes))
                else:
                    assert io == "OUT", (an, "an IN arg without data")
                    rtc.copy_nda_to_var(vs.pfx + an, poison(dims.sizes))
            rtc.run(RtcFuncCall(fn, am))
            launch = rtc.last_launch() if rtc.be == "hip" else {}
            rtc.finish_and_sync()
            what = (fop.get_func_name(), name, launch.get("kernel"), launch.get("cfg"))
            vs.check_guards()
            out = {"launch": launch}
            for an, io in spec:
                if io in ("REF", "VAL"):
                    continue
                got = rtc.copy_var_to_nda(vs.pfx + an)
                if io == "OUT":
                    out[an] = got
                else:
                    assert np.array_equal(bits(got).reshape(-1), bits(np.ascontiguousarray(d[an], got.dtype)).reshape(-1)), (what, an, "an IN arg was written")
            res[name] = out
        return res
    finally:
        rtc.finish_and_sync()
        vs.release()
        try:
            rtc.release_func(fn)
        except Exception:     # (the compile itself was refused)
            pass
        rtc.release_per_call_id_data()


# ---------------------------------------------------------------------------------------------------------------
# the references: data sets, be=cpu, the emulators (once each, read-only)
# ---------------------------------------------------------------------------------------------------------------
def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def data(cls, grad, shape):
    """(the injected classes do not depend on the gradient: one data set per shape)"""
    return _ro(gen(cls, grad if cls in FINITE else "in", tuple(shape)))


_CPU = []


def cpu_rtc():
    if not _CPU:
        r = make_rtc("(be=cpu)"); r.init(); _CPU.append(r)
    return _CPU[0]


OUT_OF = {"in": "in_grad_loss", "filts": "filts_grad_loss", "biases": "biases_grad_loss", "fb": "filts_grad_loss"}


@functools.lru_cache(maxsize=None)
def cpu_want(cls, grad, shape, bf16=False):
    """be=cpu's gradient on a class's data (through the runner: poisoned outputs, guards); `clean` is every injected class's base data."""
    d = data(cls, "filts" if grad == "fb" else grad, shape)
    w = run_fop(cpu_rtc(), func_of(grad, shape, bf16=bf16), {cls: d}, pfx="bsr_")[cls][OUT_OF[grad]]
    assert_no_poison(w, ("be=cpu", cls, grad, shape))
    w.setflags(write=False)
    return w


def bk_of(launch):
    """The K step of a launch, from its configuration string BIxBJxBK_w..."""
    return int(launch["cfg"].split("_")[0].split("x")[2])


def emu(cls, grad, shape, bk=32, ksl=1, fused=False):
    """The written chain of a launch on a class's data: in_grad_chain(BK), filts_chain(BK, KSL), biases_chain, or the fused call's biases_chain(BK, KSL)."""
    d = data(cls, "filts" if fused else grad, shape)
    g = geom_of(shape)
    if grad == "in":
        return bc.in_grad_chain(d["filts"], d["out_grad_loss"], g, bk)
    if grad == "filts":
        return bc.filts_chain(d["in"], d["out_grad_loss"], g, bk, ksl)
    with np.errstate(all="ignore"):
        return fb.biases_chain(d["out_grad_loss"], bk, ksl) if fused else bc.biases_chain(d["out_grad_loss"])


def reached(grad, shape):
    """-> bool mask of the outputs at least one real term reaches (a 1x1 at stride 2 leaves 75 % of in_grad_loss as exact +0: outside the caps)."""
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = shape
    OH, OW = out_hw(shape)
    if grad == "biases":
        return np.ones(OC, bool)
    if grad == "filts":
        m = np.zeros((KH, KW), bool)
        for fy in range(KH):
            for fx in range(KW):
                m[fy, fx] = any(0 <= oy * SY - PY + fy < H for oy in range(OH)) and any(0 <= ox * SX - PX + fx < W for ox in range(OW))
        return np.broadcast_to(m, (OC, C, KH, KW))
    my = np.array([any(0 <= y + PY - oy * SY < KH for oy in range(OH)) for y in range(H)])
    mx = np.array([any(0 <= x + PX - ox * SX < KW for ox in range(OW)) for x in range(W)])
    return np.broadcast_to(my[:, None] & mx[None, :], (B, C, H, W))


def assert_caps(cls, want, reach=None):
    """The blindness conditions on a REFERENCE result: without them a class could pass while exercising nothing.  -> the fractions."""
    w = np.asarray(want)
    fr = fractions(w[reach] if reach is not None else w)
    if cls == "wide":
        assert fr["nan"] == 0 and fr["inf"] == 0 and fr["zero"] < 0.01, fr
    elif cls == "subnormal":
        assert fr["subnormal"] >= 0.20 and fr["normal"] >= 0.20 and fr["nan"] == 0 and fr["inf"] == 0, fr
    elif cls == "overflow":
        assert 0.10 <= fr["nan"] + fr["inf"] <= 0.90, fr
    elif cls in ("nan_inf", "nan_inf_in"):
        assert fr["nan"] > 0 and fr["inf"] > 0 and 0.005 <= fr["nan"] + fr["inf"] <= 0.60, fr
    return fr


# ---------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------
def assert_bits(want, got, what=""):
    """Equal by bits; a NaN the arithmetic produced is compared as a NaN (its payload is outside the contract)."""
    want, got = np.asarray(want), np.asarray(got).reshape(np.shape(want))
    wn, gn = np.isnan(want), np.isnan(got)
    assert np.array_equal(wn, gn), (what, "NaN masks differ", int(wn.sum()), int(gn.sum()), tuple(int(v[0]) for v in np.nonzero(wn != gn)))
    bad = ~wn & (bits(want) != bits(got))
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError((what, "bits differ", int(bad.sum()), at, float(want[at]), float(got[at]), hex(int(bits(want)[at])), hex(int(bits(got)[at]))))


def kind(a):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf."""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def in_windows(shape, one):
    """One injected out_grad_loss[img, oc, oy, ox] -> (R, L), bool [B, H, W]: the in pels with y + PY - oy * SY in [0, KH) resp. in [0, SY * ceil(KH / SY)), likewise x.
    R is where the reference has a term with the element; L is the phase window of kernels/bconv_in_f32.hip, whose taps beyond the kernel are zero operands."""
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX = shape
    img, _, oy, ox, _ = one
    fy = np.arange(H) + PY - oy * SY; fx = np.arange(W) + PX - ox * SX
    R = np.zeros((B, H, W), bool); L = np.zeros((B, H, W), bool)
    R[img] = ((fy >= 0) & (fy < KH))[:, None] & ((fx >= 0) & (fx < KW))[None, :]
    L[img] = ((fy >= 0) & (fy < SY * -(-KH // SY)))[:, None] & ((fx >= 0) & (fx < SX * -(-KW // SX)))[None, :]
    return R, L


def check_in_b3(shape, d, got, clean, want, what=""):
    """The data gradient with non-finite out_grad_loss (B3).  got / clean: the kernel on the injected / the base data; want: be=cpu on the injected data.
    -> (in_grad_loss elements of L \\ R that came back non-finite, elements of L \\ R)."""
    wins = [in_windows(shape, one) for one in d["inj"]]
    R = np.any([w[0] for w in wins], axis=0); L = np.any([w[1] for w in wins], axis=0)
    C = shape[1]
    bc_ = lambda m: np.broadcast_to(m[:, None], got.shape)
    nf = ~np.isfinite(got)
    assert not np.isfinite(want[bc_(R)]).any(), (what, "the reference is finite on R: the data is not what it should be")
    assert nf[bc_(R)].all(), (what, "a pel whose chain holds an injected element came back finite", int((~nf & bc_(R)).sum()))
    assert not nf[~bc_(L)].any(), (what, "a non-finite value outside every phase window", int((nf & ~bc_(L)).sum()), tuple(int(v[0]) for v in np.nonzero(nf & ~bc_(L))))
    assert np.array_equal(bits(got)[~bc_(L)], bits(clean)[~bc_(L)]), (what, "an output outside every phase window differs from the clean run")
    for i, (Ri, _) in enumerate(wins):
        other = np.any([w[1] & ~w[0] for j, w in enumerate(wins) if j != i] + [np.zeros_like(Ri)], axis=0)
        m = bc_(Ri & ~other)
        assert np.array_equal(kind(got)[m], kind(want)[m]), (what, d["inj"][i], "NaN / +Inf / -Inf differs from the reference on R")
    leak = bc_(L & ~R)
    return int((nf & leak).sum()), int(leak.sum())


def check_filts_b3_ogl(shape, d, got, clean, want, what=""):
    """The filter gradient with non-finite out_grad_loss[img, oc, ..]: non-finite only inside the filter rows oc, at least wherever the reference is; every other
    row equals the clean run by bits.  -> (elements of those rows non-finite where the reference is finite -- padding taps --, elements of those rows)."""
    rows = np.zeros(shape[4], bool)
    rows[[one[1] for one in d["inj"]]] = True
    got = np.asarray(got).reshape(want.shape); clean = np.asarray(clean).reshape(want.shape)
    nf = ~np.isfinite(got)
    assert not nf[~rows].any(), (what, "a non-finite value outside the injected out_chans' filter rows")
    assert np.array_equal(bits(got)[~rows], bits(clean)[~rows]), (what, "a filter row of a clean out_chan differs from the clean run")
    assert nf[~np.isfinite(want)].all(), (what, "finite where the reference is not")
    return int((nf & np.isfinite(want)).sum()), int(rows.sum()) * int(np.prod(want.shape[1:]))


def check_filts_b3_in(d, got, clean, want, what=""):
    """The filter gradient with non-finite `in`: the kernel has no zero partner on that side, so the NaN / +Inf / -Inf masks are the reference's exactly and every
    other element the clean run's."""
    got = np.asarray(got).reshape(want.shape); clean = np.asarray(clean).reshape(want.shape)
    assert np.array_equal(kind(got), kind(want)), (what, "NaN / Inf masks differ from the reference", int((kind(got) != kind(want)).sum()),
                                                   tuple(int(v[0]) for v in np.nonzero(kind(got) != kind(want))))
    fin = np.isfinite(want)
    assert np.array_equal(bits(got)[fin], bits(clean)[fin]), (what, "a finite element differs from the clean run")


def check_in_b3_filts(shape, d, got, clean, want, what=""):
    """The stated exception: non-finite `filts` in the data gradient, held to containment in the injected in_chans.  -> (non-finite elements, the reference's)."""
    chans = np.zeros(shape[1], bool)
    chans[[one[1] for one in d["inj"]]] = True
    nf = ~np.isfinite(got)
    assert not nf[:, ~chans].any(), (what, "a non-finite value outside the injected in_chans")
    assert np.array_equal(bits(got)[:, ~chans], bits(clean)[:, ~chans]), (what, "a clean in_chan differs from the clean run")
    assert nf[~np.isfinite(want)].all(), (what, "finite where the reference is not")
    return int(nf.sum()), int((~np.isfinite(want)).sum())


# ---- bf16 operands: float64 on to_bf16 operands under the bound of tests/bconv_bf16_ref.py
def bf16_refs(shape, d):
    """-> {"S", "A", "W"}: (in, filts) float64 gradients on the rounded operands, on their absolute values, on the unrounded ones; non-finite operands count as 0
    (the elements they reach are not held to the bound)."""
    op = op_of(tuple(shape))
    z = lambda a: np.where(np.isfinite(a), a, F(0))
    with np.errstate(over="ignore"):
        r = [z(to_bf16(d[an])) for an in ("in", "filts", "out_grad_loss")]
    u = [z(d[an]) for an in ("in", "filts", "out_grad_loss")]
    return {"S": torch_grads(op, *r)[:2], "A": torch_grads(op, *[np.abs(a) for a in r])[:2], "W": torch_grads(op, *u)[:2]}


def check_bf16_bound(shape, which, got, r, ksl, fin=None, flush=False, with_nrms=False, what=""):
    """|got - S| <= 2 (K + KSL + 3) u A on the elements of `fin` (all by default); flush: plus (K + KSL) 2^-126, which lets any term below the normal range be lost.
    -> the largest fraction of the bound seen."""
    i = 0 if which == "in" else 1
    S, A = r["S"][i], r["A"][i]
    got = np.asarray(got, np.float64).reshape(S.shape)
    fin = np.ones(S.shape, bool) if fin is None else np.asarray(fin).reshape(S.shape)
    assert np.isfinite(got[fin]).all(), (what, which, "NaN / Inf where the reference is finite")
    K = n_terms(op_of(tuple(shape)), which)
    bound = 2.0 * (K + ksl + 3) * U * A + ((K + ksl) * 2.0 ** -126 if flush else 0.0)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - S), 0.0)
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    assert frac <= 1.0, (what, which, f"K={K} ksl={ksl}: |got - S| reaches {frac:.3f} of the bound")
    if with_nrms:
        e = nrms(got, r["W"][i])
        assert e < NRMS_BOUND, (what, which, "NRMS against the unrounded float64 gradient", e)
    return frac


def minus_zero_case(OC=1):
    """-> (shape, data): a 4 x 4 plane under a 3 x 3 / stride 1 / pad 1 filter, one in_chan, filts = +2^-100 and out_grad_loss = -2^-100 everywhere: every real
    product is -2^-200, which rounds to -0.  OC = 16: 144 terms per chain, whole K steps of 16 (no K tail); OC = 1: 9 terms and a K tail."""
    shape = (1, 1, 4, 4, OC, 3, 3, 1, 1, 1, 1)
    return shape, {"filts": np.full((OC, 1, 3, 3), 2.0 ** -100, F), "out_grad_loss": np.full((1, OC, 4, 4), -(2.0 ** -100), F), "in": np.zeros((1, 1, 4, 4), F)}


M0_TILE = "64x64x16x2x2"      # the K step of the directed case without a K tail


# ---------------------------------------------------------------------------------------------------------------
# the other backward functions (kernels/bck_ops_f32.hip): one case per function, on the smallest geometry of tests/test_bck_ops_cpu.py that has padding and a ragged
# tail.  A case runs the function under test on `rtc` and its reference on `cpu` (be=cpu), both through run_fop, and returns the launches it made:
# [(function, last_launch())].  With rtc = be=cpu a case checks its own checks (tests/test_bck_special_cpu.py).
# ---------------------------------------------------------------------------------------------------------------
import bck_ops_ref as oref
import bck_pipe_ref as pref
from boda_amd.cnn_op import add_bck_op_annotations, add_pipe_op_annotations
from test_bck_ops_cpu import ALPHA, BETA, LRN, POOL, bck_lrn_op, lrn_op, pool_op, softmax_op, spreading_op
from test_bck_pipe_cpu import concat_op, dropout_op, reduce_op

POOL_GEOM = POOL["pad_8x8_k3s2p1"]          # 3 x 4 planes of 8 x 8, 3 x 3 windows at stride 2, pad 1: 300 outputs (a ragged second workgroup), clipped border windows
LRN_GEOM = LRN["c100_ls5_5x5"]              # 100 channels in blocks of 8: a ragged last block; 650 threads
FLT_MAX = oref.FLT_MAX
_ann = lambda op, i=0: add_bck_op_annotations(op, OpTune())[i]
_pann = lambda op: add_pipe_op_annotations(op, OpTune())


def _both(rtc, cpu, fop, sets, seen, **kw):
    got = run_fop(rtc, fop, sets, pfx="bso_", **kw)
    seen += [(fop.get_func_name(), r["launch"]) for r in got.values()]
    return got, run_fop(cpu, fop, sets, pfx="bsr_", **kw)


def _outs(fop):
    return [an for an, io in pipe_func_args(fop) if io == "OUT"]


def pool_special_in():
    B, C, H, W = POOL_GEOM[:4]
    rng = np.random.default_rng(41)
    x = rng.uniform(-4, 4, (B, C, H, W)).astype(F)
    u = rng.uniform(0, 1, x.shape)
    for lo, v in ((0.00, np.nan), (0.06, np.inf), (0.09, -np.inf), (0.12, -FLT_MAX)):
        x[(u >= lo) & (u < lo + 0.03)] = v
    bits(x)[0, 1, 4, 4] = 0xFFC00001
    x[0, 0, 0:2, 0:2] = np.nan; x[1, 1, 0:2, 0:2] = -np.inf; x[2, 2, 0:2, 0:2] = -FLT_MAX; x[2, 3, 6:8, 6:8] = np.nan; x[2, 3, 7, 7] = -np.inf     # windows of NaN / -Inf / -FLT_MAX only
    return x


def case_pool_yx(rtc, cpu):
    seen = []
    sets = {"special": {"in": pool_special_in()}, "wide": {"in": _wide(np.random.default_rng(42), POOL_GEOM[:4])}}
    got, want = _both(rtc, cpu, _ann(pool_op(*POOL_GEOM)), sets, seen)
    for c in sets:
        for an in ("out", "out_in_yx"):
            assert_no_poison(got[c][an], (c, an)); assert_bits(want[c][an], got[c][an], ("hip_pool_yx", c, an))
    o, yx = got["special"]["out"], got["special"]["out_in_yx"]
    assert not np.isnan(o).any() and not np.isnan(yx).any()                          # a NaN never wins
    for at in ((0, 0, 0, 0), (1, 1, 0, 0), (2, 2, 0, 0), (2, 3, 4, 4)):              # nothing won: -FLT_MAX and -1
        assert o[at] == -FLT_MAX and yx[at] == -1.0, at
    assert np.isposinf(o).any() and ((yx >= 0) & (yx < 64)).mean() > 0.9
    assert_bits(oref.pool_yx_f32(sets["special"]["in"], *POOL_GEOM[4:])[0], o)
    ga, wa = _both(rtc, cpu, _ann(pool_op(*POOL_GEOM, avg=1, emit=0)), sets, seen)      # the average: masks equal, values by value; out_in_yx is -1
    for c in sets:
        assert_no_poison(ga[c]["out"]); assert_same(wa[c]["out"], ga[c]["out"], ("hip_pool_yx avg", c))
        assert (ga[c]["out_in_yx"] == -1.0).all()
    assert np.isnan(ga["special"]["out"]).any() and np.isinf(ga["special"]["out"]).any() and np.isfinite(ga["special"]["out"]).any()
    return seen


def spreading_sets():
    B, C, H, W, kern, stride, pad = POOL_GEOM
    rng = np.random.default_rng(43)
    out, yx = oref.pool_yx_f32(rng.uniform(-4, 4, (B, C, H, W)).astype(F), kern, stride, pad)
    ogl = rng.uniform(-2, 2, out.shape).astype(F)
    clean = {"out": out, "out_grad_loss": ogl, "out_in_yx": yx}
    yx2, ogl2 = yx.copy(), ogl.copy()
    inj = [(0, 0, 0, 0), (0, 3, 4, 4), (1, 1, 2, 3), (2, 3, 4, 4), (1, 0, 4, 0), (2, 2, 0, 2), (0, 2, 3, 1)]
    for at, v in zip(inj[:4], (np.nan, np.inf, -np.inf, np.nan)):
        ogl2[at] = v
    bits(ogl2)[inj[3]] = 0x7F800001
    for at, v in zip(inj[4:], (np.nan, -1.0, float(H * W + 5))):      # an out_in_yx that is a NaN, -1, an index past the plane: none of them matches any pel
        yx2[at] = v
    yx2[1, 2, 1, 1] = 1e9; inj.append((1, 2, 1, 1))
    return clean, {"out": out, "out_grad_loss": ogl2, "out_in_yx": yx2}, inj


def case_spreading(rtc, cpu):
    B, C, H, W, (KH, KW), (SY, SX), (PY, PX) = POOL_GEOM
    seen = []
    clean, injd, inj = spreading_sets()
    wide = dict(clean, out_grad_loss=_wide(np.random.default_rng(44), clean["out"].shape))
    held = np.zeros((B, C, H, W), bool)      # the pels a window of an injected element holds
    for b, c, oy, ox in inj:
        held[b, c, max(0, oy * SY - PY):oy * SY - PY + KH, max(0, ox * SX - PX):ox * SX - PX + KW] = True
    for avg in (0, 1):
        got, want = _both(rtc, cpu, _ann(spreading_op(*POOL_GEOM, avg=avg)), {"clean": clean, "nan_inf": injd, "wide": wide}, seen)
        for c in got:
            assert_no_poison(got[c]["in_grad_loss"], (avg, c)); assert_bits(want[c]["in_grad_loss"], got[c]["in_grad_loss"], ("hip_spreading", avg, c))
        g = got["nan_inf"]["in_grad_loss"]
        assert np.array_equal(bits(g)[~held], bits(got["clean"]["in_grad_loss"])[~held]) and np.isfinite(g[~held]).all(), (avg, "a pel no injected window holds differs from the clean run")
        assert np.isnan(g).any() and np.isinf(g).any()
        if not avg:      # the pel a changed out_in_yx pointed to has lost that window's gradient, and no other pel has gained it
            b, c, oy, ox = inj[5]
            y, x = divmod(int(clean["out_in_yx"][b, c, oy, ox]), W)
            assert got["clean"]["in_grad_loss"][b, c, y, x] != g[b, c, y, x]
    return seen


def lrn_sets():
    B, C, H, W, ls, k = LRN_GEOM
    rng = np.random.default_rng(45)
    x = rng.uniform(-30, 30, (B, C, H, W)).astype(F)
    xi = x.copy(); xi[0, 1, 2, 3] = np.nan; xi[1, 1, 4, 0] = np.inf; xi[1, 1, 0, 4] = -np.inf
    return {"clean": {"in": x}, "nan_inf": {"in": xi}, "wide": {"in": _wide(rng, x.shape)}, "subnormal": {"in": _subn(rng, x.shape)}}


def case_lrn_sb(rtc, cpu):
    """The carried sum: one Inf at channel 1 leaves Inf - Inf = NaN in ls_sum for every later channel of the pel, in the template as in the GPU's per-thread pre-walk."""
    B, C, H, W, ls, k = LRN_GEOM
    seen = []
    sets = lrn_sets()
    got, want = _both(rtc, cpu, _ann(lrn_op(B, C, H, W, ls, ALPHA, BETA, k)), sets, seen)
    for c in sets:
        for an in ("out", "out_scale_base"):
            assert_no_poison(got[c][an], (c, an))
            assert np.array_equal(kind(got[c][an]), kind(want[c][an])), ("hip_lrn_sb", c, an, "NaN / Inf masks differ from be=cpu")
        assert_bits(want[c]["out_scale_base"], got[c]["out_scale_base"], ("hip_lrn_sb", c))
        fin = np.isfinite(want[c]["out"])
        w64 = oref.lrn_out_f64(np.where(fin, sets[c]["in"], 0), np.where(fin, want[c]["out_scale_base"], 1), BETA)
        err = np.abs(np.where(fin, got[c]["out"], 0).astype(np.float64) - w64)
        assert (err <= 8 * oref.U * np.abs(w64) + 2.0 ** -149).all(), ("hip_lrn_sb out", c, float((err / (8 * oref.U * np.abs(w64) + 2.0 ** -149)).max()))
    w = want["nan_inf"]["out_scale_base"]
    for b, y, x in ((0, 2, 3), (1, 4, 0), (1, 0, 4)):      # the quirk: every later channel of the pel, not only the window's
        assert not np.isfinite(w[b, 1:, y, x]).any() and np.isfinite(w[b, 0, y, x]) == (ls // 2 < 1)
    other = np.ones((B, H, W), bool); other[0, 2, 3] = other[1, 4, 0] = other[1, 0, 4] = False
    m = np.broadcast_to(other[:, None], w.shape)
    for an in ("out", "out_scale_base"):      # every other pel: the clean run (the same kernel on the same values: the same bits)
        assert np.array_equal(bits(got["nan_inf"][an])[m], bits(got["clean"][an])[m]), ("hip_lrn_sb", an, "a clean pel differs from the clean run")
    fs = fractions(want["subnormal"]["out"])
    assert fs["subnormal"] > 0 and fs["normal"] > 0.9 and (want["subnormal"]["out_scale_base"] == F(k)).all()
    return seen


def case_bck_lrn(rtc, cpu):
    B, C, H, W, ls, k = LRN_GEOM
    seen = []
    fwd = run_fop(cpu, _ann(lrn_op(B, C, H, W, ls, ALPHA, BETA, k)), {c: s for c, s in lrn_sets().items() if c != "nan_inf"}, pfx="bsr_")
    rng = np.random.default_rng(46)
    sets = {}
    for c, s in lrn_sets().items():
        if c != "nan_inf":
            ogl = {"clean": lambda: rng.uniform(-2, 2, s["in"].shape).astype(F), "wide": lambda: _wide(rng, s["in"].shape), "subnormal": lambda: _subn(rng, s["in"].shape)}[c]()
            sets[c] = {"in": s["in"], "out": fwd[c]["out"], "out_grad_loss": ogl, "out_scale_base": fwd[c]["out_scale_base"]}
    gi = sets["clean"]["out_grad_loss"].copy(); gi[0, 1, 2, 3] = np.nan; gi[1, 1, 4, 0] = np.inf; gi[1, 97, 0, 4] = -np.inf
    sets["nan_inf"] = dict(sets["clean"], out_grad_loss=gi)
    got, want = _both(rtc, cpu, _ann(bck_lrn_op(B, C, H, W, ls, ALPHA, BETA, k)), sets, seen)
    for c in sets:
        g, w = got[c]["in_grad_loss"], want[c]["in_grad_loss"]
        assert_no_poison(g, c)
        assert np.array_equal(kind(g), kind(w)), ("hip_bck_lrn", c, "NaN / Inf masks differ from be=cpu")
        fin = np.isfinite(w)
        z = {an: np.where(np.isfinite(v), v, 0) for an, v in sets[c].items()}
        with np.errstate(invalid="ignore"):      # (wide: the carried sum cancels below zero after a large channel has left, and powf of a negative scale_base is a NaN)
            w64, S = oref.bck_lrn_f64(z["in"], z["out"], z["out_grad_loss"], z["out_scale_base"], ls, ALPHA, BETA, k)
        assert np.isfinite(w64[fin]).all() and fin.mean() > 0.5, ("hip_bck_lrn", c, "be=cpu is finite where float64 is not", float(fin.mean()))
        w64, S = np.where(fin, w64, 0), np.where(fin, S, 0)
        err = np.where(fin, np.abs(np.where(fin, g, 0).astype(np.float64) - w64), 0)
        lim = 2 * (ls + 8) * oref.U * S + (ls + 3) * 2.0 ** -149      # (the existing bound; below the normal range every one of the ls + 3 roundings is absolute)
        assert (err <= lim).all(), ("hip_bck_lrn", c, float((err / lim).max()))
    g = got["nan_inf"]["in_grad_loss"]
    other = np.ones((B, H, W), bool); other[0, 2, 3] = other[1, 4, 0] = other[1, 0, 4] = False
    m = np.broadcast_to(other[:, None], g.shape)
    assert np.array_equal(bits(g)[m], bits(got["clean"]["in_grad_loss"])[m]) and np.isnan(g).any() and np.isinf(g).any()
    assert np.isfinite(g[0, ls:, 2, 3]).all()      # nothing is carried here: the window's channels only
    return seen


SM_B, SM_C = 8, 65      # one wave per image, four waves a workgroup: two workgroups; 65 channels against 64 lanes


def softmax_sets():
    rng = np.random.default_rng(47)
    x = rng.uniform(-4, 4, (SM_B, SM_C, 1, 1)).astype(F)
    x[1, 7] = 1e30; x[2, 64] = -1e30; x[3, 64] = np.inf; x[4, 0] = -np.inf; x[5, 33] = np.nan
    label = np.array([3, -1, SM_C, 2.5, np.nan, 0, SM_C - 1, 10], F).reshape(SM_B, 1, 1)
    return x, label


def case_softmax_with_loss(rtc, cpu):
    seen = []
    x, label = softmax_sets()
    fs, fg, fl = add_bck_op_annotations(softmax_op(SM_B, SM_C), OpTune())
    got, want = _both(rtc, cpu, fs, {"x": {"in": x}}, seen, before=("prob",))
    p, wp = got["x"]["prob"], want["x"]["prob"]
    assert_no_poison(p)
    assert np.array_equal(kind(p), kind(wp)), ("hip_softmax", "NaN / Inf masks differ from be=cpu")
    assert np.isnan(wp[3]).all() and np.isnan(wp[5]).all() and np.isfinite(wp[[0, 1, 2, 4, 6, 7]]).all() and wp[1, 7] == 1.0 and wp[2, 64] == 0.0 and wp[4, 0] == 0.0
    fin = [0, 1, 2, 4, 6, 7]
    with np.errstate(all="ignore"):
        w64 = oref.softmax_f64(x[fin])
    assert (np.abs(p[fin].astype(np.float64) - w64) <= (SM_C + 8) * oref.U * w64).all(), "hip_softmax: beyond (chan + 8) u want"
    sets = {"x": {"prob": wp, "label": label}, "unmatched_only": {"prob": wp, "label": np.full((SM_B, 1, 1), -1.0, F)}}
    got, want = _both(rtc, cpu, fg, sets, seen, before=("prob",))
    for c in sets:
        g, w = got[c], want[c]
        assert_no_poison(g["in_grad_loss"]); assert_no_poison(g["loss_per_pel"])
        assert_bits(w["in_grad_loss"], g["in_grad_loss"], ("hip_sm_grad_and_loss", c))
        assert np.array_equal(kind(g["loss_per_pel"]), kind(w["loss_per_pel"])) and np.isfinite(w["loss_per_pel"]).all()
    lab = label.reshape(-1); valid = (lab >= 0) & (lab < SM_C)
    pl = np.array([wp[i, int(lab[i]), 0, 0] if valid[i] else 0.0 for i in range(SM_B)], np.float64)
    with np.errstate(invalid="ignore"):
        w64 = -np.log(np.where(pl > float(oref.FLT_MIN), pl, float(oref.FLT_MIN)))
    lpp = got["x"]["loss_per_pel"].reshape(-1)
    assert (np.abs(lpp - w64) <= 4 * oref.U * np.maximum(1.0, np.abs(w64))).all()
    floor = -oref.logf(F(oref.FLT_MIN))
    assert list(valid) == [True, False, False, True, False, True, True, True]
    # an unmatched label: -logf(FLT_MIN) by the function's own logf -- one value for all of them (inside the bound above; be=cpu's is the C library's, bit for bit),
    # and a NaN prob under a valid label gives the same: NaN > FLT_MIN is false
    lo = np.concatenate([lpp[~valid], lpp[5:6], got["unmatched_only"]["loss_per_pel"].reshape(-1)])
    assert (bits(lo) == bits(lo)[0]).all() and abs(float(lo[0]) + np.log(float(oref.FLT_MIN))) <= 4 * oref.U * 88 and (rtc.be != "cpu" or bits(lo)[0] == bits(floor))
    assert np.array_equal(bits(got["unmatched_only"]["in_grad_loss"]), bits((wp / F(SM_B)).astype(F)))                          # no channel matches: prob / img alone
    l0 = want["x"]["loss_per_pel"]
    ln = l0.copy(); ln[2] = np.nan
    li = l0.copy(); li[6] = np.inf
    sets = {"x": {"loss_per_pel": l0}, "nan": {"loss_per_pel": ln}, "inf": {"loss_per_pel": li}}
    got, want = _both(rtc, cpu, fl, sets, seen)
    for c in sets:
        assert_no_poison(got[c]["loss"]); assert_bits(want[c]["loss"], got[c]["loss"], ("hip_sum_loss_over_imgs", c))
    assert np.isnan(got["nan"]["loss"]).all() and np.isposinf(got["inf"]["loss"]).all() and np.isfinite(got["x"]["loss"]).all()
    return seen


def _specials(rng, shape):
    """U(-3, 3) with every NaN pattern, +-Inf, -0, +0 and denormals."""
    x = rng.uniform(-3, 3, shape).astype(F)
    flat = bits(x).reshape(-1)
    pats = list(NAN_BITS) + [0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0xFFFFFFFF]
    at = rng.choice(flat.size, min(flat.size, 3 * len(pats)), replace=False)
    for i, e in enumerate(at):
        flat[e] = pats[i % len(pats)]
    return flat.view(F).reshape(shape)


def case_plumbing(rtc, cpu):
    """hip_reduce, hip_concat, hip_split, hip_dropout (in place: held to the guards and to its written result only)."""
    seen = []
    rng = np.random.default_rng(48)
    n = 1023      # 255 quads and a tail of 3
    xs = [_specials(rng, (n,)) for _ in range(3)]
    for x in xs:
        x[0] = -0.0      # two (three) -0 from a +0 start: +0
    xs[0][1], xs[1][1], xs[2][1] = np.inf, -np.inf, 1.0; xs[0][2], xs[1][2], xs[2][2] = np.inf, 1.0, np.inf
    fr = _pann(reduce_op(3, f"(dims=(v={n}))"))[0]
    got, want = _both(rtc, cpu, fr, {"x": {f"ins_{i}": x for i, x in enumerate(xs)}}, seen)
    o = got["x"]["out"]
    assert_no_poison(o); assert_bits(want["x"]["out"], o, "hip_reduce")
    assert bits(o)[0] == 0 and np.isnan(o[1]) and np.isposinf(o[2])
    with np.errstate(all="ignore"):
        assert np.array_equal(kind(o), kind(((F(0) + xs[0]) + xs[1]) + xs[2]))
    B, chans, H, W = 2, (1, 2, 5), 3, 5
    ins = [_specials(rng, (B, c, H, W)) for c in chans]
    fill = np.full((B, sum(chans), H, W), 0x7FC0F00D, np.uint32).view(F)      # a third payload NaN in the ranges a call must leave alone
    wide = fill
    c0 = 0
    for f, x in zip(_pann(concat_op(B, chans, H, W)), ins):
        got, want = _both(rtc, cpu, f, {"x": {"in": x, "out": wide}}, seen)
        new = got["x"]["out"]
        assert np.array_equal(bits(new), bits(want["x"]["out"]))
        assert np.array_equal(bits(new[:, c0:c0 + x.shape[1]]), bits(x))      # NaN payloads, -0, denormals: copied bit for bit
        keep = np.ones(sum(chans), bool); keep[c0:c0 + x.shape[1]] = False
        assert np.array_equal(bits(new[:, keep]), bits(wide[:, keep]))         # every other channel range left alone
        wide = new; c0 += x.shape[1]
    for f, x in zip(_pann(concat_op(B, chans, H, W, typ="Split")), ins):
        got, want = _both(rtc, cpu, f, {"x": {"in": wide}}, seen)
        assert_no_poison(got["x"]["out"]) if not (bits(x) == POISON_BITS).any() else None
        assert np.array_equal(bits(got["x"]["out"]), bits(x)) and np.array_equal(bits(want["x"]["out"]), bits(x))
    ratio, seed = 0.5, 7
    x = _specials(rng, (2, 3, 7, 11))      # 462 elements: 115 quads and a tail of 2
    fd = _pann(dropout_op(ratio))[0]
    got, want = _both(rtc, cpu, fd, {"x": {"inout": x}}, seen, seed=seed)
    o = got["x"]["inout"]
    keep = pref.dropout_keep(x.size, ratio, seed).reshape(x.shape)
    assert (bits(o)[~keep] == 0).all() and np.isnan(x[~keep]).any()                       # a dropped NaN (or Inf, or -0) is +0
    assert np.isnan(o[keep & np.isnan(x)]).all() and np.isnan(x[keep]).any()              # a kept NaN stays a NaN
    fin = keep & ~np.isnan(x)
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(o)[fin], bits((x * F(pref.dropout_scale(ratio))).astype(F))[fin])
    assert_bits(want["x"]["inout"], o, "hip_dropout")
    return seen


CASES = {"pool_yx": case_pool_yx, "spreading": case_spreading, "lrn_sb": case_lrn_sb, "bck_lrn": case_bck_lrn, "softmax_with_loss": case_softmax_with_loss, "plumbing": case_plumbing}


# ---------------------------------------------------------------------------------------------------------------
# the launch forms of tests/test_gpu_bck_special.py, and the function ops they compile (tests/golden/ops/bck-special-ops.txt lists them: what the build pre-specialises)
# ---------------------------------------------------------------------------------------------------------------
IN_FORMS = [("planner", n, "") for n in SHAPES] + [(t, n, t) for t in ("64x128x16x2x2", "64x64x16x2x2") for n in ("3x3_s1_two_imgs_17_chans", "3x3_s2_k_not_multiple_of_s")]
KSL7 = "64x64x16x2x2x1x7"
FILTS_FORMS = [("64x64x8x2x2x1x1", n) for n in SHAPES] + [("128x128x64x2x2x1x1", n) for n in ("3x3_s1_two_imgs_17_chans", "5x5_s2_pad3_pad_ge_stride")] + \
    [("64x64x16x2x2x1x3", n) for n in SHAPES] + [(KSL7, n) for n in ("7x3_s3x2_odd_channels", "3x3_s1_img1_chan_not_32")]      # K = 36 / 81: three / six K steps over seven slices
BF_IN_FORMS = [("planner", n, "") for n in SHAPES] + [("32x32x32x1x1", n, "32x32x32x1x1") for n in ("3x3_s1_two_imgs_17_chans", "3x3_s2_k_not_multiple_of_s")]
BF_FB_FORMS = [("planner", n, "") for n in FB_SMALL] + [("64x64x32x2x2x1x7", "k1_ohw49_tail", "64x64x32x2x2x1x7")]


def other_fops():
    """The function ops of CASES, in call order."""
    B, C, H, W, ls, k = LRN_GEOM
    return [_ann(pool_op(*POOL_GEOM)), _ann(pool_op(*POOL_GEOM, avg=1, emit=0)), _ann(spreading_op(*POOL_GEOM, avg=0)), _ann(spreading_op(*POOL_GEOM, avg=1)),
            _ann(lrn_op(B, C, H, W, ls, ALPHA, BETA, k)), _ann(bck_lrn_op(B, C, H, W, ls, ALPHA, BETA, k)), *add_bck_op_annotations(softmax_op(SM_B, SM_C), OpTune()),
            _pann(reduce_op(3, "(dims=(v=1023))"))[0], *_pann(concat_op(2, (1, 2, 5), 3, 5)), *_pann(concat_op(2, (1, 2, 5), 3, 5, typ="Split")), _pann(dropout_op(0.5))[0]]


def gpu_fops():
    """Every function op the GPU file compiles."""
    out = [func_of("in", SHAPES[n], t) for _, n, t in IN_FORMS] + [func_of("in", SHAPES[n], zinp=True) for n in ("3x3_s2_k_not_multiple_of_s", "3x3_s1_two_imgs_17_chans")]
    out += [func_of("in", minus_zero_case(1)[0]), func_of("in", minus_zero_case(16)[0], M0_TILE)] + [func_of("filts", SHAPES[n], t) for t, n in FILTS_FORMS] + [func_of("biases", s) for s in SHAPES.values()]
    out += [func_of("fb", FB_SHAPES[n], t) for t, n in FB_FORMS] + [func_of("in", SHAPES[n], t, bf16=True) for _, n, t in BF_IN_FORMS]
    out += [func_of("fb", FB_SHAPES[n], t, bf16=True) for _, n, t in BF_FB_FORMS]
    return out + other_fops()
