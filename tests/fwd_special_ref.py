"""What the special-data tests of the forward convolution and sgemm kernels share (tests/test_fwd_special_cpu.py, tests/test_gpu_fwd_special.py): seeded numpy
generators of the data classes, the oracle's results on them (computed once, read-only), the blindness caps that those results must meet before a kernel's result
is looked at, runners that launch a compiled function over every class into a poisoned output with guards, and the comparison.

The contract under test is DESIGN.md section 3.0 (C1 stores, C2 finite inputs of any magnitude, C3 non-finite data).  Data classes:
  wide           magnitudes log-uniform in 2^-40 .. 2^30, random signs, ~5 % exact +0 and ~5 % -0; biases from the same distribution
  subnormal      in / filts magnitudes log-uniform in 2^-76 .. 2^-62 (products 2^-152 .. 2^-124), a few inputs themselves subnormal; biases 0 / a subnormal
  overflow       magnitudes log-uniform in 2^55 .. 2^64, random signs; finite biases
  nan_inf        U(-5, 5); 3-6 NaNs (four bit patterns) and 2-4 +-Inf in `in` (sgemm: in a and in b); filts and biases finite; no Inf in an image's last channel
  inf_last_chan  the same U(-5, 5) base with ONE +Inf, in the last channel of an image: the documented exception (a K tail that re-reads the last channel against a
                 zero filter value forms Inf * 0 = NaN); held to containment only
Comparison is by value: equal NaN masks, equal +-Inf positions and signs, == elsewhere (so -0 == +0: the kernels form fma(w, 0, acc) for padded taps, which turns a
-0 accumulator into +0; the oracle skips those taps)."""
import functools

import numpy as np

from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_codegen_annotations
from boda_amd.op import Dims, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo
from oracle import boda_oracle as bo

F = np.float32
POISON_BITS = 0x7FC0BEEF          # a NaN with a payload: no arithmetic produces it (the value tests/bn_ref.py uses)
NAN_BITS = (0x7FC00000, 0x7FFFFFFF, 0xFFC00001, 0x7F800001)
FINITE = ("wide", "subnormal", "overflow")
CLASSES = FINITE + ("nan_inf", "inf_last_chan")
OFF, EXTRA = 2, 5                 # the conv stores channels [OFF, OFF + OC) of an out of OC + EXTRA channels

# Seeds per (class, geometry) that differ from 0: chosen on the CPU (tests/test_fwd_special_cpu.py runs the caps on every shape) so that the ORACLE's result meets
# the caps below -- a statement about the data alone
SEEDS = {("wide", (2, 8, 7, 7, 16, 1, 1, 1, 1)): 5}     # (seed 0 draws zero biases: the padded border's outputs are the bias alone, 2.5 % exact zeros)
# The exponent windows of `subnormal` and `overflow` are those of a K of a few hundred terms (C * KH * KW = 150 .. 450: there the oracle gives 20 - 80 % subnormal /
# 25 - 85 % Inf outputs).  A sum of 4 or 19 terms from the same window never overflows and is hardly ever normal, and one of 496 terms nearly always: for those
# geometries the window of `in` (sgemm: of a) is moved as a whole by the number of binades below -- the smallest move, found with the oracle alone, that brings its result
# inside the caps.  Width, distribution, signs and the filts / b window stay as they are
SHIFT = {("subnormal", (3, 4, 9, 9, 33, 1, 1, 1, 0)): 3, ("overflow", (3, 4, 9, 9, 33, 1, 1, 1, 0)): 3,           # K = 4
         ("subnormal", (2, 8, 7, 7, 16, 1, 1, 1, 1)): 3, ("overflow", (2, 8, 7, 7, 16, 1, 1, 1, 1)): 3,           # K = 8
         ("subnormal", (3, 31, 4, 4, 65, 4, 4, 1, 0)): -1, ("overflow", (3, 31, 4, 4, 65, 4, 4, 1, 0)): -1,       # K = 496
         ("overflow", (5, 33, 13, 13, 70, 1, 1, 1, 0)): 1,                                                         # K = 33
         ("overflow", (100, 36, 50)): 1, ("subnormal", (33, 257, 19)): 1, ("overflow", (33, 257, 19)): 1}          # sgemm K = 50, 19

# The geometries of the GPU file's forms (tests/test_fwd_special_cpu.py holds every one of them to the caps, on the oracle and on be=cpu)
CONV_SHAPES = [(4, 20, 8, 8, 100, 3, 3, 1, 1), (3, 4, 9, 9, 33, 1, 1, 1, 0), (2, 8, 7, 7, 16, 1, 1, 1, 1), (2, 5, 17, 13, 7, 5, 5, 2, 2), (2, 3, 35, 35, 96, 11, 11, 4, 0),
               (2, 17, 9, 9, 40, 3, 3, 1, 1), (3, 3, 51, 51, 96, 11, 11, 4, 0), (4, 17, 9, 9, 70, 5, 5, 1, 2), (5, 96, 7, 7, 130, 1, 1, 1, 0), (3, 31, 4, 4, 65, 4, 4, 1, 0),
               (5, 33, 13, 13, 70, 1, 1, 1, 0), (3, 19, 11, 11, 70, 3, 3, 1, 1)]
SGEMM_GEOMS = [(100, 36, 50), (33, 257, 19), (1, 1, 1), (260, 132, 70)]
sid = lambda s: "x".join(str(v) for v in s)


def whole_input(shape):
    return shape[5] == shape[2] and shape[6] == shape[3] and shape[8] == 0


def conv_op(B, C, H, W, OC, KH, KW, S, P):
    OH = (H + 2 * P - KH) // S + 1; OW = (W + 2 * P - KW) // S + 1
    return parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C},y={KH},x={KW})),"
                    f"in=(dims=(img={B},chan={C},y={H},x={W})),in_pad=(tn=none,dims=(y={P},x={P})),kern_sz=(tn=none,dims=(y={KH},x={KW})),"
                    f"out=(dims=(img={B},chan={OC},y={OH},x={OW})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y={S},x={S}))))")


def sgemm_op(M, N, K, tn="float"):
    t = "" if tn == "float" else f"tn={tn},"
    return parse_op(f"(str_vals=(type=sgemm),nda_vals=(a=({t}dims=(K={K},M={M})),b=({t}dims=(K={K},N={N})),c=({t}dims=(M={M},N={N}))))")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def to_half(x):
    """float32 -> float16, round to nearest even; beyond the largest half it is +-Inf (numpy warns of that overflow: here it is the point)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, F).astype(np.float16)


def poison(shape):
    return np.full(shape, POISON_BITS, np.uint32).view(F)


# ---------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------
def _logu(rng, shape, lo, hi):
    """Magnitudes 2^U(lo, hi) with random signs, as float32 (the power is formed in float64 and rounded once)."""
    m = np.exp2(rng.uniform(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)
    return m.astype(F)


def _wide(rng, shape):
    v = _logu(rng, shape, -40, 30)
    u = rng.uniform(0, 1, shape)
    v[u < 0.05] = F(0.0)
    v[(u >= 0.05) & (u < 0.10)] = F(-0.0)
    return v


def _subn(rng, shape, few=True, shift=0):
    v = _logu(rng, shape, -76 + shift, -62 + shift)
    if few and v.size:     # a few elements that are themselves subnormal: any of the patterns 0x00000001 .. 0x007FFFFF, either sign
        n = max(1, v.size // 50)
        at = rng.choice(v.size, n, replace=False)
        pat = rng.integers(1, 0x00800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31)
        v.reshape(-1)[at] = pat.view(F)
    return v


def _u5(rng, shape):
    return rng.uniform(-5, 5, shape).astype(F)


def _put(arr, idx, pattern):
    bits(arr)[idx] = np.uint32(pattern)


def _rng(cls, geom, seed):
    if seed is None:
        seed = SEEDS.get((cls, tuple(geom)), 0)
    return np.random.default_rng([seed, CLASSES.index(cls) if cls in CLASSES else 9] + [int(v) for v in geom])


def gen_conv(cls, shape, seed=None):
    """-> {"in", "filts", "biases", "inj": [(img, chan, y, x, kind)]} for the geometry (B, C, H, W, OC, KH, KW, S, P)."""
    B, C, H, W, OC, KH, KW, S, P = shape
    rng = _rng("nan_inf" if cls == "inf_last_chan" else cls, shape, seed)     # (inf_last_chan: nan_inf's base data)
    si, sf = (B, C, H, W), (OC, C, KH, KW)
    inj = []
    if cls == "wide":
        x, f, b = _wide(rng, si), _wide(rng, sf), _wide(rng, (OC,))
    elif cls == "subnormal":
        x, f = _subn(rng, si, shift=SHIFT.get((cls, tuple(shape)), 0)), _subn(rng, sf, few=False)
        b = np.zeros(OC, F)
        odd = np.arange(OC) % 2 == 1
        b[odd] = (rng.integers(1, 0x00800000, int(odd.sum())).astype(np.uint32) | (rng.integers(0, 2, int(odd.sum())).astype(np.uint32) << 31)).view(F)
    elif cls == "overflow":
        sh = SHIFT.get((cls, tuple(shape)), 0)
        x, f, b = _logu(rng, si, 55 + sh, 64 + sh), _logu(rng, sf, 55, 64), _u5(rng, (OC,))
    elif cls in ("nan_inf", "inf_last_chan"):
        x, f, b = _u5(rng, si), _u5(rng, sf), _u5(rng, (OC,))
        base = x.copy()
        if cls == "inf_last_chan":
            at = (B // 2, C - 1, H // 2, W // 2)
            _put(x, at, 0x7F800000); inj.append(at + ("+inf",))
        else:
            assert C >= 2, "nan_inf keeps its Infs out of the last channel: C >= 2"
            # the places that go wrong: first image / first channel / corner pel, the pel before an image boundary, the last image's last pel, a border pel; then random ones
            # (a whole-input window makes every output of an image with an injected element non-finite: there the NaNs go into the first image and the Infs into the
            # last, so that the images between stay clean)
            whole = KH == H and KW == W and P == 0
            # (the fourth: the first channel of the last image, which a K tail that ran on into the next image would read)
            nan_at = [(0, 0, 0, 0), (0, C - 1, H - 1, W - 1), (0 if whole else B - 1, C - 1, H - 1, W - 2 if whole else W - 1), (0 if whole else B - 1, 0, H // 2, W // 2)]
            for _ in range(int(rng.integers(0, 3))):     # 4 - 6 in all
                nan_at.append((0 if whole else int(rng.integers(0, B)), int(rng.integers(0, C)), int(rng.integers(0, H)), int(rng.integers(0, W))))
            inf_at = [(B - 1 if whole else 0, 0, H - 1, W // 2, +1), (B - 1, C - 2, H // 2, 0, -1)]     # border pels of the first and the last image
            for _ in range(int(rng.integers(0, 3))):     # 2 - 4 in all
                inf_at.append((B - 1 if whole else int(rng.integers(0, B)), int(rng.integers(0, C - 1)), int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.choice([-1, 1]))))
            for i, at in enumerate(nan_at):
                _put(x, at, NAN_BITS[i % 4]); inj.append(at + ("nan",))
            for *at, sg in inf_at:
                if tuple(at) in nan_at:
                    continue
                _put(x, tuple(at), 0x7F800000 if sg > 0 else 0xFF800000); inj.append(tuple(at) + ("+inf" if sg > 0 else "-inf",))
    else:
        raise ValueError(cls)
    d = {"in": x, "filts": f, "biases": b, "inj": inj}
    if cls in ("nan_inf", "inf_last_chan"):
        d["base_in"] = base
    return d


def gen_sgemm(cls, geom, seed=None):
    """-> {"a": [K, M], "b": [K, N], "inj"} for the geometry (M, N, K)."""
    M, N, K = geom
    rng = _rng(cls, geom, seed)
    sa, sb = (K, M), (K, N)
    inj = []
    if cls == "wide":
        a, b = _wide(rng, sa), _wide(rng, sb)
    elif cls == "subnormal":
        a, b = _subn(rng, sa, shift=SHIFT.get((cls, tuple(geom)), 0)), _subn(rng, sb, few=False)
    elif cls == "overflow":
        sh = SHIFT.get((cls, tuple(geom)), 0)
        a, b = _logu(rng, sa, 55 + sh, 64 + sh), _logu(rng, sb, 55, 64)
    elif cls == "nan_inf":
        a, b = _u5(rng, sa), _u5(rng, sb)
        if a.size < 8 or b.size < 8:     # (1, 1, 1): one of each is all there is room for
            _put(a, (0, 0), NAN_BITS[1]); _put(b, (K - 1, N - 1), 0x7F800000); inj = [("a", 0, 0, "nan"), ("b", K - 1, N - 1, "+inf")]
        else:
            n = 0
            for name, arr, cols in (("a", a, M), ("b", b, N)):
                at = [(0, 0), (K - 1, cols - 1)] + [(int(rng.integers(0, K)), int(rng.integers(0, cols))) for _ in range(1 + int(rng.integers(0, 2)))]     # 3 - 4 NaNs a side
                for p in at:
                    _put(arr, p, NAN_BITS[n % 4]); n += 1; inj.append((name,) + p + ("nan",))
                for sg in ((+1, -1) if name == "a" else (-1,)):     # 3 Infs in all
                    p = (int(rng.integers(0, K)), int(rng.integers(0, cols)))
                    if p in at:
                        continue
                    _put(arr, p, 0x7F800000 if sg > 0 else 0xFF800000); inj.append((name,) + p + ("+inf" if sg > 0 else "-inf",))
    else:
        raise ValueError(cls)
    return {"a": a, "b": b, "inj": inj}


def gen_sgemm_half(geom, seed=0):
    """The half-typed variant for the half-storage sgemm (fp32 math on half operands, c rounded to half once) -> {cls: {"a", "b"}} as float16:
      big        operands up to 2^9: sums of K products beyond 65504 must store as +-Inf
      subnormal  operands around 2^-10 .. 2^-8 and subnormal halves (below 2^-14): results among the subnormal halves and below
      nan        U(-5, 5) with a NaN in a, a NaN in b and an Inf in a."""
    M, N, K = geom
    rng = np.random.default_rng([seed, 16, M, N, K])
    H = np.float16
    out = {}
    out["big"] = {"a": _logu(rng, (K, M), 3, 9).astype(H), "b": _logu(rng, (K, N), 3, 9).astype(H)}
    a = _logu(rng, (K, M), -12, -6).astype(H); b = _logu(rng, (K, N), -12, -6).astype(H)
    a.reshape(-1)[::7] = (rng.integers(1, 0x0400, a.reshape(-1)[::7].size).astype(np.uint16)).view(H)     # subnormal halves
    out["subnormal"] = {"a": a, "b": b}
    a = _u5(rng, (K, M)).astype(H); b = _u5(rng, (K, N)).astype(H)
    a[0, 0] = H(np.nan); b[K - 1, N - 1] = H(np.nan); a[K // 2, M // 2] = H(np.inf)
    out["nan"] = {"a": a, "b": b}
    return out


# ---------------------------------------------------------------------------------------------------------------
# the oracle's side: results (once per geometry and class, read-only) and the blindness caps
# ---------------------------------------------------------------------------------------------------------------
def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def conv_data(cls, shape):
    return _ro(gen_conv(cls, tuple(shape)))


@functools.lru_cache(maxsize=None)
def conv_want(cls, shape, relu):
    d = conv_data(cls, shape)
    S, P = shape[7], shape[8]
    w = bo.conv_fwd(d["in"], d["filts"], d["biases"], (S, S), (P, P), bool(relu))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def conv_clean(shape, relu):
    """nan_inf's and inf_last_chan's base data without the injected elements, through the oracle."""
    d = conv_data("nan_inf", shape)
    S, P = shape[7], shape[8]
    return bo.conv_fwd(d["base_in"], d["filts"], d["biases"], (S, S), (P, P), bool(relu))


@functools.lru_cache(maxsize=None)
def sgemm_data(cls, geom):
    return _ro(gen_sgemm(cls, tuple(geom)))


@functools.lru_cache(maxsize=None)
def sgemm_want(cls, geom):
    d = sgemm_data(cls, geom)
    w = bo.sgemm(d["a"], d["b"])
    w.setflags(write=False)
    return w


def window_mask(shape, inj, ext=0):
    """-> bool [B, OH, OW]: the output pels whose window holds an injected element.  ext: the window grown by that many rows / columns on every side."""
    B, C, H, W, OC, KH, KW, S, P = shape
    OH = (H + 2 * P - KH) // S + 1; OW = (W + 2 * P - KW) // S + 1
    m = np.zeros((B, OH, OW), bool)
    for img, _, y, x, _ in inj:
        for oy in range(OH):
            for ox in range(OW):
                if -ext <= y - (oy * S - P) < KH + ext and -ext <= x - (ox * S - P) < KW + ext:
                    m[img, oy, ox] = True
    return m


def fractions(want):
    """-> the fractions of an oracle result (ReLU off) that the caps speak of."""
    w = np.asarray(want, F).reshape(-1)
    a = np.abs(w)
    tiny = np.finfo(F).tiny
    return {"nan": float(np.isnan(w).mean()), "inf": float(np.isinf(w).mean()), "zero": float((w == 0).mean()),
            "subnormal": float(((a > 0) & (a < tiny)).mean()), "normal": float((np.isfinite(w) & (a >= tiny)).mean())}


MIN_OUTPUTS_FOR_CAPS = 16     # a fraction of fewer outputs says nothing (sgemm 1 x 1 x 1 has one): such geometries run every class, the caps are not applied to them


def assert_caps(cls, want, whole_input=False):
    """The blindness conditions, on the oracle's result alone (ReLU off): without them a class could pass while exercising nothing.
    whole_input: every output of an image has the whole image as its window, so one injected element makes all of that image's outputs non-finite; with injections
    in the first and the last image the 60 % cap cannot hold for three images -- the condition is then that at least one image is non-finite and one is clean."""
    fr = fractions(want)
    if np.asarray(want).size < MIN_OUTPUTS_FOR_CAPS:
        return fr
    if cls == "wide":
        assert fr["nan"] == 0 and fr["inf"] == 0 and fr["zero"] < 0.01, fr
    elif cls == "subnormal":
        assert fr["subnormal"] >= 0.20 and fr["normal"] >= 0.20 and fr["nan"] == 0 and fr["inf"] == 0, fr
    elif cls == "overflow":
        assert 0.10 <= fr["inf"] <= 0.90, fr
    elif cls == "nan_inf":
        nf = fr["nan"] + fr["inf"]
        assert fr["nan"] > 0 and fr["inf"] > 0, fr
        if whole_input:
            per_img = ~np.isfinite(np.asarray(want)).reshape(want.shape[0], -1)
            assert per_img.all(axis=1).any() and (~per_img.any(axis=1)).any(), fr
        else:
            assert 0.005 <= nf <= 0.60, fr
    elif cls == "inf_last_chan":
        assert fr["inf"] > 0 and fr["nan"] == 0 and (whole_input or fr["inf"] <= 0.60), fr
    return fr


# ---------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------
def assert_same(want, got, what=""):
    """Equal by value: the same NaN mask, the same +-Inf positions and signs, == on every other element (-0 == +0)."""
    want, got = np.asarray(want), np.asarray(got)
    assert want.shape == got.shape and want.dtype == got.dtype, (what, want.shape, got.shape, want.dtype, got.dtype)
    wn, gn = np.isnan(want), np.isnan(got)
    assert np.array_equal(wn, gn), (what, "NaN masks differ", int(wn.sum()), int(gn.sum()), _first(wn != gn, want, got))
    wi, gi = np.isinf(want), np.isinf(got)
    assert np.array_equal(wi, gi), (what, "Inf masks differ", int(wi.sum()), int(gi.sum()), _first(wi != gi, want, got))
    ok = wn | (want == got)
    assert ok.all(), (what, "values differ", int((~ok).sum()), _first(~ok, want, got))


def _first(bad, want, got):
    at = tuple(int(v[0]) for v in np.nonzero(bad))
    return at, float(want[at]), float(got[at])


def assert_contained(want, got, what="", relu=False):
    """inf_last_chan: non-finite exactly where the oracle is non-finite, equal elsewhere -> how many of the oracle's Infs came back as the same Inf / as NaN.
    relu: the ReLU turns a NaN into 0 (in the oracle as in the kernels), so the exception's NaN -- Inf * 0 in a K tail that re-reads the last channel -- arrives as 0
    where the oracle has +Inf: there, and only there, a 0 counts as that NaN."""
    want, got = np.asarray(want), np.asarray(got)
    wf, gf = np.isfinite(want), np.isfinite(got)
    squashed = ~wf & (got == 0) if relu else np.zeros(want.shape, bool)
    assert np.array_equal(~wf, ~gf | squashed), (what, "non-finite outputs differ", int((~wf).sum()), int((~gf).sum()), _first(~wf != (~gf | squashed), want, got))
    ok = ~wf | (want == got)
    assert ok.all(), (what, "values differ", int((~ok).sum()), _first(~ok, want, got))
    wi = np.isinf(want)
    same = int((wi & (got == want)).sum()); nan = int((wi & (np.isnan(got) | squashed)).sum())
    assert same + nan == int(wi.sum()), (what, "an Inf came back with the other sign")
    return same, nan


def assert_c3_against_clean(clean, got, mask, what=""):
    """C3's last clause: outside the windows that hold an injected element every output equals the clean run (mask [B, OH, OW] over got [B, OC, OH, OW])."""
    m = np.broadcast_to(mask[:, None], got.shape)
    assert np.isfinite(got[~m]).all() and np.array_equal(got[~m], clean[~m]), (what, "an output whose window holds no injected element differs from the clean run")


# ---------------------------------------------------------------------------------------------------------------
# runners
# ---------------------------------------------------------------------------------------------------------------
GUARD = np.full(4, POISON_BITS, np.uint32)


class _Vars:
    """Vars with a 4-float guard var behind each (tests/bn_ref.run_func says what such a guard can show: a write to a wrong var, not a small overrun)."""

    def __init__(self, rtc, pfx):
        self.rtc, self.pfx, self.made = rtc, pfx, []

    def make(self, an, dims):
        vn = self.pfx + an
        self.rtc.create_var_with_dims(vn, dims); self.made.append(vn)
        self.rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); self.made.append(vn + "_guard")
        self.rtc.copy_nda_to_var(vn + "_guard", GUARD.view(F))
        return vn

    def check_guards(self):
        for vn in self.made:
            if vn.endswith("_guard"):
                assert np.array_equal(bits(self.rtc.copy_var_to_nda(vn)), GUARD), (vn, "a guard var was written")

    def release(self):
        for vn in self.made:
            self.rtc.release_var(vn)


def run_conv(rtc, shape, datasets, relus=(1, 0), tile="", wide=True, tune=None, func="hip_conv", before_run=None):
    """Compile the annotated op once per ReLU setting, create the vars once, then for every data set {cls: {"in", "filts", "biases"}} and ReLU setting: upload, refill
    `out` with the poison, run.  wide: `out` has OC + EXTRA channels and the conv stores through out_chan_off = OFF (be=hip); otherwise exact dims (be=cpu takes no
    other).  tune: an OpTune (the bf16-operand function); tile: the conv_tile tune of the launch.
    -> {(cls, relu): {"out": the conv's channel slice, "launch": last_launch()}}.  Asserted here, for every run: the guard channels and the guard vars hold the poison
    bit for bit, the inputs read back unchanged."""
    B, C, H, W, OC = shape[:5]
    op = conv_op(*shape)
    res = {}
    vs = _Vars(rtc, "fsc_")
    funcs = []
    try:
        annos = {}
        for relu in relus:
            anno = add_codegen_annotations(op, tune or OpTune())
            assert anno.get_func_name() == func, anno.get_func_name()
            anno.nda_vals["conv_has_relu"].v = (int(relu),)
            fn = f"fs_conv_r{int(relu)}"
            rtc.compile([RtcFuncInfo(fn, "", [a for a, _ in NATIVE_ARGS[func]], anno)]); funcs.append(fn)
            annos[relu] = anno
        anno = annos[relus[0]]
        od = anno.get_dims("out")
        odims = Dims.make("float", img=B, chan=OC + EXTRA, y=od.dsz("y"), x=od.dsz("x")) if wide else od
        am = {an: RtcArg.var(vs.make(an, anno.get_dims(an))) for an in ("in", "filts", "biases")}
        am["out"] = RtcArg.var(vs.make("out", odims))
        am["stride"] = RtcArg.ref(anno.get_dims("stride")); am["in_pad"] = RtcArg.ref(anno.get_dims("in_pad"))
        if wide:
            am["out_chan_off"] = RtcArg.scalar(OFF, "uint32_t")
        for cls, d in datasets.items():
            for an in ("in", "filts", "biases"):
                rtc.copy_nda_to_var(vs.pfx + an, d[an])
            for relu in relus:
                rtc.copy_nda_to_var(vs.pfx + "out", poison(odims.sizes))
                if rtc.be == "hip":
                    rtc.set_tune("conv_tile", tile)
                if before_run:
                    before_run()
                try:
                    rtc.run(RtcFuncCall(f"fs_conv_r{int(relu)}", am)); rtc.finish_and_sync()
                finally:
                    if rtc.be == "hip":
                        rtc.set_tune("conv_tile", "")
                launch = rtc.last_launch() if rtc.be == "hip" else {}
                got = rtc.copy_var_to_nda(vs.pfx + "out")
                what = (shape, cls, relu, launch.get("kernel"), launch.get("cfg"))
                if wide:
                    gb = bits(got)
                    assert (gb[:, :OFF] == POISON_BITS).all() and (gb[:, OFF + OC:] == POISON_BITS).all(), (what, "a store outside the channel slice")
                    got = np.ascontiguousarray(got[:, OFF:OFF + OC])
                vs.check_guards()
                for an in ("in", "filts", "biases"):
                    assert np.array_equal(bits(rtc.copy_var_to_nda(vs.pfx + an)).reshape(-1), bits(d[an]).reshape(-1)), (what, an, "an IN arg was written")
                res[(cls, relu)] = {"out": got, "launch": launch}
        return res
    finally:
        rtc.finish_and_sync()
        vs.release()
        for fn in funcs:
            rtc.release_func(fn)
        rtc.release_per_call_id_data()


def run_sgemm(rtc, geom, datasets, tile="", tn="float"):
    """The twin for sgemm: c NaN-prefilled with its exact dims, a guard var behind every var, a and b read back unchanged.  datasets {cls: {"a", "b"}}
    -> {cls: {"c", "launch"}}."""
    op = sgemm_op(*geom, tn=tn)
    npt = np.float16 if tn == "half" else F
    pz = np.full(1, 0x7EEF, np.uint16).view(np.float16)[0] if tn == "half" else poison((1,))[0]     # (half: a NaN with a payload too)
    anno = add_codegen_annotations(op, OpTune())
    assert anno.get_func_name() == "hip_sgemm"
    res = {}
    vs = _Vars(rtc, "fsg_")
    try:
        rtc.compile([RtcFuncInfo("fs_sgemm", "", ["a", "b", "c"], anno)])
        am = {an: RtcArg.var(vs.make(an, anno.get_dims(an))) for an in "abc"}
        cd = anno.get_dims("c")
        for cls, d in datasets.items():
            for an in "ab":
                rtc.copy_nda_to_var(vs.pfx + an, np.ascontiguousarray(d[an], npt))
            rtc.copy_nda_to_var(vs.pfx + "c", np.full(cd.sizes, pz, npt))
            if rtc.be == "hip":
                rtc.set_tune("sgemm_tile", tile)
            try:
                rtc.run(RtcFuncCall("fs_sgemm", am)); rtc.finish_and_sync()
            finally:
                if rtc.be == "hip":
                    rtc.set_tune("sgemm_tile", "")
            launch = rtc.last_launch() if rtc.be == "hip" else {}
            got = rtc.copy_var_to_nda(vs.pfx + "c")
            what = (geom, cls, launch.get("kernel"), launch.get("cfg"))
            vs.check_guards()
            for an in "ab":
                assert np.array_equal(bits(rtc.copy_var_to_nda(vs.pfx + an)).reshape(-1), bits(np.ascontiguousarray(d[an], npt)).reshape(-1)), (what, an, "an IN arg was written")
            res[cls] = {"c": got, "launch": launch}
        return res
    finally:
        rtc.finish_and_sync()
        vs.release()
        rtc.release_func("fs_sgemm"); rtc.release_per_call_id_data()


def assert_no_poison(got, what=""):
    b = bits(got)
    p = POISON_BITS if b.dtype == np.uint32 else 0x7EEF
    assert not (b == p).any(), (what, "an output element was never stored", int((b == p).sum()), tuple(int(v[0]) for v in np.nonzero(b == p)))


BF16_POISON = 0x7FEF              # the bf16 twin of POISON_BITS; read back through the layout pass it is the float 0x7FEF0000


def run_nhwc(rtc, shape, datasets, tune, relus=(1, 0), tile=""):
    """The channels-last bf16 runner: the host arrays go into the `<arg>_ref` vars (reference layout, float) and the project's own layout passes fill the kernel's
    tensors and bring `out` back -- the host never re-implements a layout.  `out` is prefilled with a payload NaN of its own type, a guard var sits behind every var.
    -> {(cls, relu): {"out": float NCHW, "launch"}}; asserted here: guards, `in_ref` / `filts_ref` / `biases` unchanged."""
    from boda_amd import nhwc
    from boda_amd.cnn_op import pipe_func_args
    op = conv_op(*shape)
    nhwc.ensure_compiled(rtc)
    res = {}
    vs = _Vars(rtc, "fsn_")
    funcs = []
    try:
        annos = {}
        for relu in relus:
            anno = add_codegen_annotations(op, tune)
            assert anno.get_func_name() == "hip_conv_nhwc", anno.get_func_name()
            anno.nda_vals["conv_has_relu"].v = (int(relu),)
            fn = f"fs_nhwc_r{int(relu)}"
            rtc.compile([RtcFuncInfo(fn, "", [a for a, _ in pipe_func_args(anno)], anno)]); funcs.append(fn)
            annos[relu] = anno
        anno = annos[relus[0]]
        am, refd = {}, {}
        for an, io in pipe_func_args(anno):
            if io == "REF":
                am[an] = RtcArg.ref(anno.get_dims(an)); continue
            d = anno.get_dims(an); rd = anno.get_dims(an + "_ref") if anno.has(an + "_ref") else d
            am[an] = RtcArg.var(vs.make(an, d))
            if rd != d:
                vs.make(an + "_ref", rd); refd[an] = rd
        od = anno.get_dims("out")
        fill = np.full(od.sizes, BF16_POISON, np.uint16) if od.tn == "bfloat16" else poison(od.sizes)
        for cls, d in datasets.items():
            for an in ("in", "filts", "biases"):
                if an in refd:
                    rtc.copy_nda_to_var(vs.pfx + an + "_ref", d[an])
                    rtc.run(nhwc.xpose_call(an, vs.pfx + an + "_ref", vs.pfx + an, refd[an], anno.get_dims(an), anno))
                else:
                    rtc.copy_nda_to_var(vs.pfx + an, d[an])
            for relu in relus:
                rtc.copy_nda_to_var(vs.pfx + "out", fill)
                rtc.set_tune("conv_tile", tile)
                try:
                    rtc.run(RtcFuncCall(f"fs_nhwc_r{int(relu)}", am)); rtc.finish_and_sync()
                finally:
                    rtc.set_tune("conv_tile", "")
                launch = rtc.last_launch()
                if "out" in refd:
                    rtc.run(nhwc.xpose_call("out", vs.pfx + "out_ref", vs.pfx + "out", refd["out"], od, anno)); rtc.finish_and_sync()
                    got = rtc.copy_var_to_nda(vs.pfx + "out_ref")
                else:
                    got = rtc.copy_var_to_nda(vs.pfx + "out")
                what = (shape, cls, relu, launch.get("kernel"), launch.get("cfg"))
                vs.check_guards()
                for an in ("in", "filts", "biases"):
                    vn = vs.pfx + an + ("_ref" if an in refd else "")
                    assert np.array_equal(bits(rtc.copy_var_to_nda(vn)).reshape(-1), bits(d[an]).reshape(-1)), (what, an, "an IN arg was written")
                res[(cls, relu)] = {"out": got, "launch": launch, "out_tn": od.tn}
        return res
    finally:
        rtc.finish_and_sync()
        vs.release()
        for fn in funcs:
            rtc.release_func(fn)
        rtc.release_per_call_id_data()
