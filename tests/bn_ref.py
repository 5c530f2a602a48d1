"""What the training-BatchNorm tests share (tests/test_bn_cpu.py, tests/test_gpu_bn.py): the numpy twin of the five functions' written formulas and of the chain of
their per-channel sums (boda_amd/csrc/kernels/bn_f32.hip), inputs, a runner for a bare function with NaN-filled outputs and guard vars, and
the float64 bounds.

The twin is the written formula on np.float32 arrays, one numpy operation per rounding.  The chain of a sum over a channel's elements e = img * HW + pel:
slabs of `slab` elements; inside a slab chain t (of 256) owns the elements with (r / 4) mod 256 == t and adds them to +0 in ascending r; the chains meet in the tree
h = 128 .. 1: a[t] += a[t + h]; the slab partials are added in slab order starting from the first.  Every equality is np.array_equal on the uint32 views."""
import numpy as np

from boda_amd.cnn_op import bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, fan_out_func_op, pipe_func_args
from boda_amd.op import Dims
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo

F = np.float32
U = 2.0 ** -24
GUARD_BITS = 0x7FC0BEEF
EPS, MAF = 1e-5, 0.9

# (img, chan, y, x): the smallest shapes at which each path can go wrong
SHAPES = [(1, 1, 1, 1), (2, 3, 1, 1), (2, 4, 2, 2), (3, 5, 3, 3), (3, 2, 7, 7), (5, 65, 4, 4), (2, 3, 57, 57)]
# forced slab lengths (0: the planner's).  2,3,57,57 under 2000: N = 6498 -> slabs of 2000, 2000, 2000 and a ragged 498; the edge at 2000 lies inside a plane
# (3249 pels), the slab [2000, 4000) runs across the two images.  The small shapes get edges inside a plane, at a plane's end and quads that straddle two images
FORCED = {(2, 3, 57, 57): (0, 2000, 1024), (2, 4, 2, 2): (0, 4), (3, 5, 3, 3): (0, 4, 12), (3, 2, 7, 7): (0, 48, 100), (5, 65, 4, 4): (0, 16), (2, 3, 1, 1): (0,), (1, 1, 1, 1): (0, 4)}
CASES = [(s, slab) for s in SHAPES for slab in FORCED[s]]
case_id = lambda c: "x".join(map(str, c[0])) + f"_slab{c[1]}"


def dims_of(shape):
    return Dims.make("float", img=shape[0], chan=shape[1], y=shape[2], x=shape[3])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def slab_plan(C, N, forced=0):
    """The twin of bn_slab_plan (csrc/rtc_types.h) -> (slab, nslabs)."""
    if forced:
        slab = forced
    else:
        want = max(1, -(-512 // C))
        slab = -(-N // want)
        slab = -(-slab // 1024) * 1024
        slab = max(slab, 4096)
    return slab, max(1, -(-N // slab))


def chain_sum(terms, slab):
    """The written chain over one channel's terms (float32, in element order) -> np.float32.  Padding a slab with +0 terms changes no bit: a chain starts at +0, so it
    is never -0, and x + +0 = x."""
    terms = np.asarray(terms, F).reshape(-1)
    parts = []
    for e0 in range(0, terms.size, slab):
        t = terms[e0:e0 + slab]
        t = np.concatenate([t, np.zeros((-t.size) % 1024, F)]).reshape(-1, 256, 4)   # (round, chain, element of the quad)
        acc = np.zeros(256, F)
        for r in range(t.shape[0]):
            for j in range(4):
                acc = acc + t[r, :, j]
        h = 128
        while h:
            acc[:h] = acc[:h] + acc[h:2 * h]
            h >>= 1
        parts.append(F(acc[0]))
    s = parts[0]
    for p in parts[1:]:
        s = F(s + p)
    assert s.dtype == F
    return s


def chan_terms(a, c):
    return np.ascontiguousarray(a[:, c]).reshape(-1)


def stats_np(x, run_mean, run_var, eps=EPS, maf=MAF, forced=0):
    """-> mean, inv_std, run_mean', run_var'."""
    B, C, H, W = x.shape
    N = B * H * W
    slab, _ = slab_plan(C, N, forced)
    fN, omm = F(N), F(1) - F(maf)
    unb = fN / F(N - 1) if N > 1 else F(1)
    mean = np.zeros(C, F); istd = np.zeros(C, F); rm = np.zeros(C, F); rv = np.zeros(C, F)
    for c in range(C):
        xc = chan_terms(x, c)
        m = chain_sum(xc, slab) / fN
        d = xc - m
        var = chain_sum(d * d, slab) / fN
        ve = var + F(eps)
        sd = np.sqrt(ve)
        mean[c] = m; istd[c] = F(1) / sd
        rm[c] = F(maf) * run_mean[c] + omm * m
        uv = var if N == 1 else var * unb
        rv[c] = F(maf) * run_var[c] + omm * uv
        assert all(v.dtype == F for v in (m, var, ve, sd, uv))
    return mean, istd, rm, rv


def bc(v):
    return np.asarray(v, F).reshape(1, -1, 1, 1)


def fwd_np(x, mean, istd, scale, bias, relu):
    d = x - bc(mean)
    xh = d * bc(istd)
    y = xh * bc(scale)
    y = y + bc(bias)
    if relu:
        y = np.where(y > 0, y, F(0))
    assert y.dtype == F
    return y


def bck_sums_np(x, mean, istd, dy, forced=0):
    B, C, H, W = x.shape
    slab, _ = slab_plan(C, B * H * W, forced)
    xh = (x - bc(mean)) * bc(istd)
    t = dy * xh
    sg = np.array([chain_sum(chan_terms(t, c), slab) for c in range(C)], F)
    bg = np.array([chain_sum(chan_terms(dy, c), slab) for c in range(C)], F)
    return sg, bg


def bck_in_np(x, mean, istd, scale, sg, bg, dy):
    B, C, H, W = x.shape
    fN = F(B * H * W)
    k = np.asarray(scale, F) * np.asarray(istd, F)
    mb = np.asarray(bg, F) / fN
    mg = np.asarray(sg, F) / fN
    xh = (x - bc(mean)) * bc(istd)
    t1 = dy - bc(mb)
    t2 = xh * bc(mg)
    t3 = t1 - t2
    dx = bc(k) * t3
    assert dx.dtype == F
    return dx


def make_inputs(shape, seed=0):
    """x and dy of both signs (x off-centre, so that mean matters), the last channel of x a constant, scale of both signs and an exact zero, a non-trivial running pair."""
    B, C, H, W = shape
    rng = np.random.default_rng([seed, 77, B, C, H, W])
    x = (rng.standard_normal(shape) * 1.5 + 0.4).astype(F)
    x[:, C - 1] = F(0.75)
    dy = rng.standard_normal(shape).astype(F)
    scale = rng.uniform(0.5, 1.5, C).astype(F) * np.where(np.arange(C) % 2 == 0, 1, -1).astype(F)
    if C > 2:
        scale[1] = 0.0
    bias = rng.uniform(-0.5, 0.5, C).astype(F)
    run_mean = rng.uniform(-1, 1, C).astype(F)
    run_var = rng.uniform(0.5, 2, C).astype(F)
    return dict(x=x, dy=dy, scale=scale, bias=bias, run_mean=run_mean, run_var=run_var)


def run_func(rtc, fop, ins, repeat=1, keep=None, bind=None):
    """Compile the function op, give every arg a var (OUT args filled with NaN, a 4-float guard var behind each), upload `ins` {arg: array}, run `repeat` times -> ({arg:
    array} of every OUT / INOUT arg after each run, as a list), and check the guards.  bind {arg: arg}: the first arg shares the second's var.
    What the guards can and cannot show: a guard is an allocation of its own (the var bound to an arg must have exactly the op's dims, so it cannot live inside a wider
    var), and a store a few elements past a tensor would most likely land in the allocator's padding, not in it.  They catch a write to a wrong var, not a small
    overrun.  What covers the tensors themselves is the NaN prefill (an element left unwritten stays NaN and fails the comparison) and bit equality with be=cpu and numpy
    on every element; that the inputs came back unchanged is checked below."""
    spec = pipe_func_args(fop)
    bind = bind or {}
    rtc.compile([RtcFuncInfo("bn_f", "", [a for a, _ in spec], fop)])
    made, am = [], {}
    guard = np.full(4, GUARD_BITS, np.uint32).view(F)
    try:
        for an, io in spec:
            if an in bind:
                continue
            vn = "bnv_" + an
            d = fop.get_dims(an)
            rtc.create_var_with_dims(vn, d); made.append(vn); am[an] = RtcArg.var(vn)
            rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); made.append(vn + "_guard")
            rtc.copy_nda_to_var(vn + "_guard", guard)
            rtc.copy_nda_to_var(vn, np.ascontiguousarray(ins[an], F).reshape(d.sizes) if an in ins else np.full(d.sizes, np.nan, F))
        for an, to in bind.items():
            am[an] = am[to]
        call = RtcFuncCall("bn_f", am)
        res = []
        for _ in range(repeat):
            rtc.run(call)
            rtc.finish_and_sync()
            res.append({an: rtc.copy_var_to_nda(am[an].n) for an, io in spec if io != "IN"})
        if keep is not None:
            keep.append(rtc.last_launch() if rtc.be == "hip" else {})
        for vn in made:
            if vn.endswith("_guard"):
                assert np.array_equal(rtc.copy_var_to_nda(vn).view(np.uint32), np.full(4, GUARD_BITS, np.uint32)), vn
        for an, io in spec:
            if io == "IN" and an in ins and an not in bind.values():
                assert same_bits(rtc.copy_var_to_nda(am[an].n).reshape(-1), np.asarray(ins[an], F).reshape(-1)), (an, "an IN arg was written")
        return res
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("bn_f"); rtc.release_per_call_id_data()


def run_all_five(rtc, shape, forced=0, relu=1, seed=0, repeat=1):
    """The five functions on one backend, each fed the BACKEND's own upstream results -> dict of everything."""
    d = dims_of(shape)
    i = make_inputs(shape, seed)
    r = dict(i)
    keep = []
    sts = run_func(rtc, bn_stats_func_op(d, EPS, MAF, forced), {"in": i["x"], "run_mean": i["run_mean"], "run_var": i["run_var"]}, repeat=repeat, keep=keep)
    for s in sts[1:]:     # (the running pair moves on; the batch statistics must not)
        assert same_bits(s["mean"], sts[0]["mean"]) and same_bits(s["inv_std"], sts[0]["inv_std"]), "a repeated launch on the same workspace changed bits"
    st = sts[0]
    r["launch_stats"] = keep[0]
    r.update(mean=st["mean"], inv_std=st["inv_std"], run_mean2=st["run_mean"], run_var2=st["run_var"])
    common = {"in": i["x"], "mean": r["mean"], "inv_std": r["inv_std"]}
    r["out"] = run_func(rtc, bn_fwd_func_op(d, relu), dict(common, scale=i["scale"], bias=i["bias"]))[0]["out"]
    sums = run_func(rtc, bn_bck_sums_func_op(d, forced), dict(common, out_grad_loss=i["dy"]), repeat=repeat)
    for s in sums[1:]:
        assert same_bits(s["scale_grad_loss"], sums[0]["scale_grad_loss"]) and same_bits(s["bias_grad_loss"], sums[0]["bias_grad_loss"]), "a repeated launch on the same workspace changed bits"
    r.update(sg=sums[0]["scale_grad_loss"], bg=sums[0]["bias_grad_loss"])
    r["dx"] = run_func(rtc, bn_bck_in_func_op(d), dict(common, scale=i["scale"], scale_grad_loss=r["sg"], bias_grad_loss=r["bg"], out_grad_loss=i["dy"]))[0]["in_grad_loss"]
    return r


def check_against_numpy(r, shape, forced=0, relu=1):
    """Every result of run_all_five against the twin, each stage fed the twin's own upstream results (equal bits upstream make them the backend's too)."""
    mean, istd, rm, rv = stats_np(r["x"], r["run_mean"], r["run_var"], EPS, MAF, forced)
    assert same_bits(r["mean"], mean), "mean"
    assert same_bits(r["inv_std"], istd), "inv_std"
    assert same_bits(r["run_mean2"], rm) and same_bits(r["run_var2"], rv), "running pair"
    assert same_bits(r["out"], fwd_np(r["x"], mean, istd, r["scale"], r["bias"], relu)), "out"
    sg, bg = bck_sums_np(r["x"], mean, istd, r["dy"], forced)
    assert same_bits(r["sg"], sg) and same_bits(r["bg"], bg), "bck sums"
    assert same_bits(r["dx"], bck_in_np(r["x"], mean, istd, r["scale"], sg, bg, r["dy"])), "dx"


# ---- float64 bounds: one u = 2^-24 per written operation, on the float64 formula evaluated with the backend's own fp32 mean, inv_std and sums
TINY = 2.0 ** -149
INFL = 1.0 + 1e-6     # (the second-order terms of (1 + u)^k)


def f64_bounds_fractions(r, shape, relu=0):
    """-> {name: the largest observed fraction of its bound}; asserts nothing.  r: run_all_five's (relu as run there).
    out:  d = x - m [u], xh = d * is [u], y1 = xh * sc [u], y = y1 + b [u]:   |err| <= u * (3 |P| + |P + b|) <= u * (4 |P| + |b|),  P = d * is * sc
    dx:   k = sc * is [u], mb = bg / N [u], mg = sg / N [u], xh [2u], t1 = dy - mb [u], t2 = xh * mg [u], t3 = t1 - t2 [u], dx = k * t3 [u]:
          |err| <= |k| * u * (|mb| + |t1| + 4 |t2| + |t3|) + 2 u |k * t3|
    sums: |got - want| <= 2 (N + 3) u SUM |term|, for any order."""
    D = np.float64
    x, dy = r["x"].astype(D), r["dy"].astype(D)
    B, C, H, W = shape
    N = B * H * W
    m, s = bc(r["mean"]).astype(D), bc(r["inv_std"]).astype(D)
    sc, bi = bc(r["scale"]).astype(D), bc(r["bias"]).astype(D)
    fr = {}
    P = (x - m) * s * sc
    want = P + bi
    bound = U * (4 * np.abs(P) + np.abs(bi)) * INFL + TINY
    if relu:
        want = np.where(want > 0, want, 0.0)
    fr["out"] = float(np.max(np.abs(r["out"].astype(D) - want) / bound))
    xh = (x - m) * s
    k = sc * s; mb = bc(r["bg"]).astype(D) / N; mg = bc(r["sg"]).astype(D) / N
    t1 = dy - mb; t2 = xh * mg; t3 = t1 - t2
    bound = (np.abs(k) * U * (np.abs(mb) + np.abs(t1) + 4 * np.abs(t2) + np.abs(t3)) + 2 * U * np.abs(k * t3)) * INFL + TINY
    fr["dx"] = float(np.max(np.abs(r["dx"].astype(D) - k * t3) / bound))
    ax = (0, 2, 3)
    for name, got, term in (("S1", r["mean"].astype(D) * N, x + 0 * m), ("S2", None, (x - m) ** 2), ("scale_grad", r["sg"].astype(D), dy * xh), ("bias_grad", r["bg"].astype(D), dy + 0 * m)):
        if got is None:
            continue     # (S2 is not an output: var + eps is, through inv_std -- checked by the bit-exact twin)
        tol = 2.0 * (N + 3) * U * np.abs(term).sum(axis=ax) + TINY
        extra = U * np.abs(got) if name == "S1" else 0.0     # (mean * N undoes a division that rounded once)
        fr[name] = float(np.max(np.abs(got - term.sum(axis=ax)) / (tol + extra)))
    return fr


# ---- the residual pipe and its float64 walk
import bck_pipe_ref as ref
from boda_amd.conv_pipe import ConvPipe, PipeOp

N_CLASS = 5
RES_SEEDS = (2477, 8679, 9116)     # data / param seeds of the residual pipe for which the float64 walk passes its guards: the first three of 0 .. 9116 (see test_bn_cpu.py)
RES_SEED = RES_SEEDS[0]
# the largest max|got - want| / max|want| over the nodes of the residual pipe and the three seeds, measured on be=cpu against the float64 walk (1.129e-06, 2.465e-06,
# 1.261e-06; tests/test_bn_cpu.py prints them).  Both backends are held to ten times this besides the cap 5e-4
DRIVER_DEV_CPU = 2.465e-06


def residual(B=3):
    """3 images of 9 x 9: a stem conv + BatchNorm + Scale + ReLU; a bottleneck block with a projection shortcut (branch1) and one with an identity shortcut, 8 - 16
    channels, every convolution followed by BatchNorm + Scale, 2a / 2b by a ReLU as well, res = ReLU(shortcut + 2c); global average pool, fc, loss."""
    p = ConvPipe("residual", "data", Dims.make("float", img=B, chan=3, y=9, x=9))

    def cbs(tag, bot, oc, k, s=1, pad=0, relu=True):
        p.add(PipeOp(tag, "Convolution", bot, tag, out_chans=oc, kern_sz=(k, k), stride=(s, s), in_pad=(pad, pad)))
        p.add(PipeOp("bn_" + tag, "BatchNorm", tag, tag)); p.add(PipeOp("scale_" + tag, "Scale", tag, tag))
        if relu:
            p.add(PipeOp(tag + "_relu", "ReLU", tag, tag))
        return tag
    cbs("stem", "data", 8, 3, 1, 1)
    short = cbs("a_b1", "stem", 16, 1, relu=False)
    t = cbs("a_2a", "stem", 8, 1); t = cbs("a_2b", t, 8, 3, 1, 1); t = cbs("a_2c", t, 16, 1, relu=False)
    p.add(PipeOp("res_a", "Eltwise", short, "res_a", bots=(short, t))); p.add(PipeOp("res_a_relu", "ReLU", "res_a", "res_a"))
    t = cbs("b_2a", "res_a", 8, 1); t = cbs("b_2b", t, 8, 3, 1, 1); t = cbs("b_2c", t, 16, 1, relu=False)
    p.add(PipeOp("res_b", "Eltwise", "res_a", "res_b", bots=("res_a", t))); p.add(PipeOp("res_b_relu", "ReLU", "res_b", "res_b"))
    p.add(PipeOp("gap", "Pooling", "res_b", "gap", kern_sz=None, avg_pool=1))
    p.add(PipeOp("fc", "Convolution", "gap", "fc", out_chans=N_CLASS, kern_sz=(1, 1)))
    return p


def res_params(cp, seed=RES_SEED):
    """He-scaled filters, small biases, scale of both signs away from zero, a running pair away from (0, 1)."""
    rng = np.random.default_rng([seed, 7])
    out = {}
    for n, d in cp.params.items():
        if n.endswith("_filts"):
            out[n] = (rng.standard_normal(d.sizes) * np.sqrt(2.0 / (d.dsz("in_chan") * d.dsz("y") * d.dsz("x")))).astype(F)
        elif n.endswith("_scale"):
            out[n] = (rng.uniform(0.6, 1.4, d.sizes) * rng.choice([-1.0, 1.0], d.sizes)).astype(F)
        elif n.endswith("_var"):
            out[n] = rng.uniform(0.5, 1.5, d.sizes).astype(F)
        else:
            out[n] = rng.uniform(-0.3, 0.3, d.sizes).astype(F)
    return out


def res_inputs(cp, seed=RES_SEED):
    rng = np.random.default_rng([seed, 11])
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(F)
    label = rng.integers(0, N_CLASS, (data.shape[0], 1, 1)).astype(F)
    return data, label


def net_bn_f64(cp, params, data, label, guard_rel=1e-4, only_loss=False):
    """bck_pipe_ref.net_f64 extended with the three op types (and cut down to what the residual pipe holds): a float64 forward and backprop with a TRAINING BatchNorm
    -- batch mean and biased variance, y = (x - mean) / sqrt(var + eps) --, Scale y * scale + bias, Eltwise SUM.  Same guards: no ReLU input within guard_rel max|v| of zero.
    -> {<node>_grad_loss (with respect to the node's value BEFORE its in-place ops), <param>_grad_loss, loss, and <bn-tag>_batch_mean / _batch_var}."""
    f64 = lambda a: np.asarray(a, np.float64)
    ax = (0, 2, 3)
    val = {cp.in_node: f64(data)}
    keep, res = {}, {}
    for o in cp.ops:
        x = val[o.bot]
        if o.type == "Convolution":
            keep[o.tag] = x
            val[o.top] = ref.conv_f64(x, f64(params[o.tag + "_filts"]), f64(params[o.tag + "_biases"]), o.stride, o.in_pad)
        elif o.type == "ReLU":
            if np.min(np.abs(x)) < guard_rel * np.max(np.abs(x)):
                raise AssertionError(f"net_f64 guard: ReLU {o.tag} has an input within {guard_rel} max|v| of zero")
            keep[o.tag] = x > 0
            val[o.top] = np.where(x > 0, x, 0.0)
        elif o.type == "Pooling":
            assert o.avg_pool
            d = cp.nodes[o.top]
            out, arg = ref.pool_f64(x, (d.dsz("y"), d.dsz("x")), o.kern_sz, o.stride, o.in_pad, 1, 0.0)
            keep[o.tag] = (x.shape, arg); val[o.top] = out
        elif o.type == "BatchNorm":
            m = x.mean(axis=ax, keepdims=True); v = ((x - m) ** 2).mean(axis=ax, keepdims=True)
            istd = 1.0 / np.sqrt(v + float(F(o.eps)))
            xh = (x - m) * istd
            keep[o.tag] = (xh, istd); val[o.top] = xh
            res[o.tag + "_batch_mean"] = m.reshape(-1); res[o.tag + "_batch_var"] = v.reshape(-1)
        elif o.type == "Scale":
            keep[o.tag] = x
            val[o.top] = x * f64(params[o.tag + "_scale"]).reshape(1, -1, 1, 1) + f64(params[o.tag + "_bias"]).reshape(1, -1, 1, 1)
        elif o.type == "Eltwise":
            val[o.top] = sum(val[b] for b in o.bots)
        else:
            raise AssertionError(o.type)
    B = data.shape[0]
    lab = np.asarray(label).reshape(B).astype(int)
    t = cp.out_node()
    z = val[t].reshape(B, -1)
    e = np.exp(z - z.max(axis=1, keepdims=True)); p = e / e.sum(axis=1, keepdims=True)
    res["loss"] = float(-np.log(p[np.arange(B), lab]).mean())
    if only_loss:
        return res
    p[np.arange(B), lab] -= 1.0
    grad = {t: (p / B).reshape(val[t].shape)}
    for o in reversed(cp.ops):
        og = grad[o.top]
        if o.type == "Convolution":
            gx, gf, gb = ref.conv_bck_f64(keep[o.tag], f64(params[o.tag + "_filts"]), og, o.stride, o.in_pad)
            res[o.tag + "_filts_grad_loss"] = gf; res[o.tag + "_biases_grad_loss"] = gb
            grad[o.bot] = grad.get(o.bot, 0.0) + gx
        elif o.type == "ReLU":
            grad[o.top] = np.where(keep[o.tag], og, 0.0)
        elif o.type == "Pooling":
            shp, arg = keep[o.tag]
            grad[o.bot] = grad.get(o.bot, 0.0) + ref.pool_bck_f64(shp, og, arg, o.kern_sz, o.stride, o.in_pad, 1)
        elif o.type == "Scale":
            res[o.tag + "_scale_grad_loss"] = (og * keep[o.tag]).sum(axis=ax); res[o.tag + "_bias_grad_loss"] = og.sum(axis=ax)
            grad[o.top] = og * f64(params[o.tag + "_scale"]).reshape(1, -1, 1, 1)
        elif o.type == "BatchNorm":
            xh, istd = keep[o.tag]
            grad[o.top] = istd * (og - og.mean(axis=ax, keepdims=True) - xh * (og * xh).mean(axis=ax, keepdims=True))
        elif o.type == "Eltwise":
            for b in o.bots:
                grad[b] = grad.get(b, 0.0) + og
    for n, g in grad.items():
        res[n + "_grad_loss"] = g
    return res
