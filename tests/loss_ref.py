"""The full SoftmaxWithLoss (csrc/kernels/loss_f32.hip): the numpy twins of hip_softmax_loss_fwd / hip_loss_norm / hip_softmax_loss_bck -- the same
fp32 operations in the same order; exp and log are numpy's, so prob and loss_per_pel are held to bounds and everything behind them to bits -- the float64 formulas of
the semantics, the shapes, label sets and data of the issue, the bounds, and a runner for one bare function with NaN-filled outputs and guard vars.

Bounds (u = 2^-24), derived as in the header of tests/test_gpu_bck_ops.py:
    prob            (C + 8) u want + 2^-148          any order of C positive terms, expf, one divide; the second term is fp32's underflow floor (two roundings onto
                                                     the subnormal grid, spacing 2^-149), without which no fp32 softmax of +-80 logits can meet a relative bound
    loss_per_pel    4 u max(1, |want|)               one logf, against -log in float64 of the call's OWN stored prob[L]
    gradient        s ((C + 8) u p + 4 u |p - d|) + 2^-147   prob's bound carried through (p - d) * s, two roundings of its own and the divide that made s
    loss            (depth + 2) u SUM|lpp| + SUM(per-pel bound) / Z;  depth = ceil(N / 256) + 8, the written chain of hip_loss_norm
"""
import numpy as np

from boda_amd.bck_graph import LossSpec
from boda_amd.cnn_op import NATIVE_ARGS
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

F = np.float32
U = 2.0 ** -24
FLT_MIN = F(1.175494351e-38)
INVALID_LOSS = F(-np.log(np.float64(FLT_MIN)))   # 126 ln 2 correctly rounded: 0x42AEAC50, the constant both backends store
assert INVALID_LOSS.view(np.uint32) == 0x42AEAC50

# (B, C, y, x) -> the form the planner picks (y * x >= 64: pel).  2,5,9,7 has 63 pels per plane and so takes the WAVE form under that rule; 2,5,9,9 (162 pels) is what
# it was meant to cover in the pel form: a partial wave and a partial workgroup
SHAPES = [((2, 5, 9, 7), "wave"), ((2, 5, 9, 9), "pel"), ((3, 21, 16, 17), "pel"), ((2, 1, 8, 8), "pel"), ((1, 70, 8, 8), "pel"), ((1, 3, 1, 63), "wave"), ((5, 1, 1, 1), "wave"), ((5, 63, 1, 1), "wave"),
          ((5, 64, 1, 1), "wave"), ((5, 65, 1, 1), "wave"), ((4, 1000, 1, 1), "wave"), ((2, 70, 2, 3), "wave")]
BIG = (3, 21, 16, 17)
NORMS = ("valid", "full", "batch_size", "none")
WEIGHTS = (1.0, 0.3, 0.0)
DATA = ("pm4", "wide", "low")
SID = lambda s: "x".join(map(str, s))


def form_of(shape):
    return "pel" if shape[2] * shape[3] >= 64 else "wave"


def logits(shape, kind="pm4", seed=0):
    """pm4: the uniform +-4 of test_bck_ops_cpu.softmax_in (the same numbers on a 1 x 1 plane); wide: +-80; low: every logit in [-210, -190]."""
    lo, hi = {"pm4": (-4.0, 4.0), "wide": (-80.0, 80.0), "low": (-210.0, -190.0)}[kind]
    return np.random.default_rng(seed + 17 * shape[1] + shape[0]).uniform(lo, hi, shape).astype(F)


def label_sets(shape, seed=0):
    """-> [(name, label float img:y:x, ignore_label or None, the number of ignored pels it was meant to have)], fixed seeds."""
    B, C, H, W = shape
    n = B * H * W
    rng = np.random.default_rng([seed, B, C, H, W])
    base = rng.integers(0, C, n).astype(F)
    third = rng.permutation(n)[:max(1, n // 3)]
    out = [("valid", base.copy(), None, 0)]
    for ig in (255, 0, -1):
        lab = base.copy()
        if ig == 0:   # a real class: every other pel gets another class where there is one
            lab = (rng.integers(1, C, n) if C > 1 else np.zeros(n)).astype(F)
        lab[third] = ig
        out.append((f"ign{ig}", lab, ig, n if (ig == 0 and C == 1) else third.size))
    out.append(("all_ignored", np.full(n, 255, F), 255, n))
    for nm, bad in (("invalid_C", F(C)), ("invalid_nan", F(np.nan))):
        lab = base.copy(); lab[int(rng.integers(0, n))] = bad
        out.append((nm, lab, None, 0))
    return [(nm, lab.reshape(B, H, W), ig, cnt) for nm, lab, ig, cnt in out]


def classes(label, C, spec):
    """-> (ignored, valid, L) per pel under the kernels' tests; L = -1 where not valid."""
    lab = np.asarray(label, F)
    ignored = (lab == F(spec.ignore_label)) if spec.ignore_label is not None else np.zeros(lab.shape, bool)
    with np.errstate(invalid="ignore"):
        valid = ~ignored & (lab >= 0) & (lab < F(C))
    L = np.where(valid, np.nan_to_num(lab, nan=0.0, posinf=0.0, neginf=0.0), -1).astype(np.int64)
    return ignored, valid, np.where(valid, L, -1)


# ---- the fp32 twins
def _butterfly(v, op):
    """The xor butterfly over axis 0 (64 lanes): at step k lane l takes op(partner, own); both orders give one word for max and add."""
    for k in (32, 16, 8, 4, 2, 1):
        idx = np.arange(64) ^ k
        v = op(v[idx], v)
    return v[0]


def exp_diff(a, m):
    """exp(a - m) with the difference held exactly as the pair (d, r) of the two-sum: the kernel's exp_diff."""
    a, m = np.asarray(a, F), np.asarray(m, F)
    d = (a - m).astype(F); bb = (d - a).astype(F)
    r = ((a - (d - bb).astype(F)).astype(F) - (m + bb).astype(F)).astype(F)
    e = np.exp(d).astype(F)
    return (e + (e * r).astype(F)).astype(F)


def fwd_f32(x, label, spec):
    """hip_softmax_loss_fwd's operations: the pel form's sequential chain over the channels, or the wave form's 64 lane chains and butterflies.  -> (prob, loss_per_pel)"""
    x = np.asarray(x, F); B, C, H, W = x.shape
    pick = lambda o, a: np.where(o > a, o, a)
    if form_of(x.shape) == "pel":
        m = x[:, 0].copy()
        for c in range(1, C):
            m = pick(x[:, c], m)
        S = np.zeros_like(m)
        for c in range(C):
            S = (S + exp_diff(x[:, c], m)).astype(F)
    else:
        lm = np.full((64,) + m_shape(x), -np.inf, F); ls = np.zeros((64,) + m_shape(x), F)
        for c in range(C):
            lm[c % 64] = pick(x[:, c], lm[c % 64])
        m = _butterfly(lm, pick)
        for c in range(C):
            ls[c % 64] = (ls[c % 64] + exp_diff(x[:, c], m)).astype(F)
        S = _butterfly(ls, lambda o, a: (a + o).astype(F))
    prob = (exp_diff(x, np.broadcast_to(m[:, None], x.shape)) / S[:, None]).astype(F)
    return prob, lpp_of_prob_f32(prob, label, spec)


def m_shape(x):
    return (x.shape[0], x.shape[2], x.shape[3])


def lpp_of_prob_f32(prob, label, spec):
    ignored, valid, L = classes(label, prob.shape[1], spec)
    pl = np.take_along_axis(prob, np.maximum(L, 0)[:, None], axis=1)[:, 0]
    v = (-np.log(np.maximum(pl, FLT_MIN))).astype(F)
    return np.where(ignored, F(0), np.where(valid, v, INVALID_LOSS)).astype(F)


def chain_depth(n_pels):
    return -(-n_pels // 256) + 8


def norm_f32(label, lpp, spec):
    """hip_loss_norm's chain: thread t sums pels t, t + 256, ... from +0, then the halving tree.  -> (loss float 1x1, state float 4 = Z, s, count, sum)"""
    lab = np.asarray(label, F); B = lab.shape[0]; n = lab.size
    v = np.zeros(-(-n // 256) * 256, F); v[:n] = np.asarray(lpp, F).ravel()
    a = np.zeros(256, F)
    for row in v.reshape(-1, 256):
        a = (a + row).astype(F)
    h = 128
    while h:
        a[:h] = (a[:h] + a[h:2 * h]).astype(F); h //= 2
    ssum = F(a[0])
    ignored = (lab == F(spec.ignore_label)) if spec.ignore_label is not None else np.zeros(lab.shape, bool)
    count = int(n - ignored.sum())
    Z = F({"valid": max(1, count), "full": n, "batch_size": B, "none": 1}[spec.normalization])
    s = F(F(spec.weight) / Z)
    return np.array([[F(ssum / Z)]], F), np.array([Z, s, F(count), ssum], F)


def bck_f32(prob, label, state, spec):
    """hip_softmax_loss_bck: ignored ? +0 : (prob - [c == L]) * s, s = state[1]; two roundings."""
    prob = np.asarray(prob, F); C = prob.shape[1]
    ignored, valid, L = classes(label, C, spec)
    hit = (np.arange(C)[None, :, None, None] == L[:, None]) & valid[:, None]
    d = np.where(hit, (prob - F(1)).astype(F), prob)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (d * F(state[1])).astype(F)
    return np.where(ignored[:, None], F(0), g).astype(F)


# ---- float64
def softmax_f64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def lpp_f64(prob, label, spec):
    """-log(max(prob[L], FLT_MIN)) in float64 of the prob GIVEN; +0 at ignored pels, -log(FLT_MIN) at invalid ones."""
    ignored, valid, L = classes(label, prob.shape[1], spec)
    pl = np.take_along_axis(np.asarray(prob, np.float64), np.maximum(L, 0)[:, None], axis=1)[:, 0]
    return np.where(ignored, 0.0, np.where(valid, -np.log(np.maximum(pl, np.float64(FLT_MIN))), -np.log(np.float64(FLT_MIN))))


def loss_f64(x, label, spec):
    """The semantics in float64 on the fp32 logits -> dict(prob, lpp, count, Z, s, loss, grad); s from the fp32 weight."""
    p = softmax_f64(x); B, C, H, W = p.shape
    ignored, valid, L = classes(label, C, spec)
    lpp = lpp_f64(p, label, spec)
    count = int(ignored.size - ignored.sum())
    Z = float({"valid": max(1, count), "full": ignored.size, "batch_size": B, "none": 1}[spec.normalization])
    s = float(F(spec.weight)) / Z
    delta = ((np.arange(C)[None, :, None, None] == L[:, None]) & valid[:, None]).astype(np.float64)
    grad = np.where(ignored[:, None], 0.0, (p - delta) * s)
    return dict(prob=p, lpp=lpp, count=count, Z=Z, s=s, loss=lpp.sum() / Z, grad=grad, delta=delta, ignored=ignored)


def prob_bound(want, C):
    return (C + 8) * U * want + 2.0 ** -148


def lpp_bound(want):
    return 4 * U * np.maximum(1.0, np.abs(want))


def grad_bound(w, C):
    return abs(w["s"]) * ((C + 8) * U * w["prob"] + 4 * U * np.abs(w["prob"] - w["delta"])) + (2.0 ** -147 if w["s"] else 0.0)


def loss_bound(w, C):
    """(depth + 2) u SUM|lpp| for the chain and the divide, and per pel prob's relative error (C + 8) u (what it moves -log by) plus logf's 4 u max(1, |lpp|); all over Z."""
    n = w["lpp"].size
    per_pel = np.where(w["ignored"], 0.0, (C + 8) * U + lpp_bound(w["lpp"]))
    return ((chain_depth(n) + 2) * U * np.abs(w["lpp"]).sum() + per_pel.sum()) / w["Z"]


# ---- bits
def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- one bare function through the C ABI: NaN-filled outputs, a 4-float guard var in front of and behind every var
GUARD = np.array([0x5A5A0001, 0x5A5A0002, 0x5A5A0003, 0x5A5A0004], np.uint32).view(F)
POISON = np.uint32(0x7FC0BEEF)   # a payload NaN


def run_func(rtc, fop, ins, kernel=None, pfx="lt_"):
    """Compile and run one annotated function with host inputs -> {OUT arg: array}.  Every OUT var is filled with a payload NaN first; asserted: no guard word changed,
    every IN var still holds its input's bits, and (kernel given: be=hip) the launch was that kernel."""
    fn = fop.get_func_name()
    spec = NATIVE_ARGS[fn]
    rtc.compile([RtcFuncInfo(pfx + "f", "", [a for a, _ in spec], fop)])
    made = []

    def var(vn, d):
        rtc.create_var_with_dims(vn, d); made.append(vn)
    try:
        for an, io in spec:
            d = fop.get_dims(an)
            var(pfx + an + "_g0", Dims.make("float", v=4)); var(pfx + an, d); var(pfx + an + "_g1", Dims.make("float", v=4))
            for g in ("_g0", "_g1"):
                rtc.copy_nda_to_var(pfx + an + g, GUARD)
            rtc.copy_nda_to_var(pfx + an, np.ascontiguousarray(ins[an], F).reshape(d.sizes) if io == "IN" else np.full(d.sizes, POISON, np.uint32).view(F))
        rtc.run(RtcFuncCall(pfx + "f", {an: RtcArg.var(pfx + an) for an, _ in spec}))
        rtc.finish_and_sync()
        if kernel is not None:
            assert rtc.last_launch()["kernel"] == kernel, rtc.last_launch()
        outs = {}
        for an, io in spec:
            for g in ("_g0", "_g1"):
                assert bits_eq(rtc.copy_var_to_nda(pfx + an + g), GUARD), (fn, an, g)
            got = rtc.copy_var_to_nda(pfx + an)
            if io == "IN":
                assert bits_eq(got, np.ascontiguousarray(ins[an], F).reshape(got.shape)), (fn, an, "an input was written")
            else:
                assert not np.any(bits(got) == POISON), (fn, an, "a poisoned word survived")
                outs[an] = got
        return outs
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(pfx + "f"); rtc.release_per_call_id_data()


def bare_run(rtc, fop, dims=None, pfx="lb_"):
    """Compile one function, create its vars (dims: {arg: Dims} in place of the op's) and run it on whatever they hold: for the refusals."""
    spec = NATIVE_ARGS[fop.get_func_name()]
    rtc.compile([RtcFuncInfo(pfx + "f", "", [a for a, _ in spec], fop)])
    made = []
    try:
        for an, _ in spec:
            rtc.create_var_with_dims(pfx + an, (dims or {}).get(an, fop.get_dims(an))); made.append(pfx + an)
        rtc.run(RtcFuncCall(pfx + "f", {an: RtcArg.var(pfx + an) for an, _ in spec}))
        rtc.finish_and_sync()
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(pfx + "f")


KERNELS = {"hip_softmax_loss_fwd": "bodahip_softmax_loss_fwd", "hip_loss_norm": "bodahip_loss_norm", "hip_softmax_loss_bck": "bodahip_softmax_loss_bck"}


def dims_of(shape):
    return Dims(("img", "chan", "y", "x"), tuple(shape), "float")


def golden_specs():
    """The specs of tests/golden/ops/loss-ops.txt: per shape the three functions under LossSpec(0.3, 255, "valid"); on the first shape also every other normalisation
    without an ignore_label, and ignore_label -1."""
    from boda_amd.cnn_op import loss_norm_func_op, softmax_loss_bck_func_op, softmax_loss_fwd_func_op
    ctors = (softmax_loss_fwd_func_op, loss_norm_func_op, softmax_loss_bck_func_op)
    out = []
    for shape, _ in SHAPES:
        out += [c(dims_of(shape), LossSpec(0.3, 255, "valid")) for c in ctors]
    for nz in NORMS[1:]:
        out += [c(dims_of(SHAPES[0][0]), LossSpec(1.0, None, nz)) for c in ctors]
    out += [c(dims_of(SHAPES[0][0]), LossSpec(0.0, -1, "valid")) for c in ctors]
    return out
