"""What the input-transform tests share (tests/test_data_transform_cpu.py, tests/test_gpu_data_transform.py): the numpy twin of hip_data_transform, written from the rule
csrc/kernels/data_f32.hip states (clamps included), the case lists, a runner for the bare function with typed vars and guard vars, the refusals with their sentences, and
the checks of the two drivers, all of which take the backend as an argument.

Equality is on the bytes.  Every value is two IEEE operations on exact inputs, so no tolerance appears; where the twin has a NaN the backend must have a NaN (sign and
payload are the platform's)."""
import itertools

import numpy as np
import pytest

import bn_ref
import eval_ref as E
import solver_ref as V
from boda_amd.bck_pipe import ConvPipeBck, Solver, add_bck_ops
from boda_amd.cnn_op import data_transform_func_op, pipe_func_args
from boda_amd.conv_pipe import ConvPipe, PipeOp, _conv
from boda_amd.eval_pipe import EvalPipe
from boda_amd.input_pipe import DATA_RAW_VAR, DATA_XF_MEAN_VAR, DATA_XF_PLAN_VAR, DATA_XF_TAG, InputTransform
from boda_amd.op import Dims, Nda, Op, RtErr, UnsupErr
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo
from test_bck_pipe_cpu import N_CLASS, PIPES, small_params

F, U8, U32 = np.float32, np.uint8, np.uint32
GUARD_BITS = E.GUARD_BITS
NP_OF = {"float": F, "uint32_t": U32, "uint8_t": U8}
GARBAGE = 0xA5A5F00D     # plan word 3


# ---- the twin
def data_transform_np(src, plan, mean, scale, crop, layout):
    """hip_data_transform: src uint8 (B, H, W, C) ("hwc") or (B, C, H, W) ("chw"), plan uint32 (B, 4), mean float32 (C,) or (C, H, W), crop = (ch, cw) -> float32
    (B, C, ch, cw).  Per element: yo = min(plan[i][0], H - ch), xo = min(plan[i][1], W - cw), m = plan[i][2] != 0, sy = yo + y, sx = xo + (cw - 1 - x if m else x),
    d = fp32(src - mu), out = fp32(d * scale)."""
    src = np.asarray(src, U8); plan = np.asarray(plan, U32); mean = np.asarray(mean, F); scale = F(scale)
    chw = src if layout == "chw" else src.transpose(0, 3, 1, 2)
    B, C, H, W = chw.shape
    ch, cw = crop
    assert plan.shape == (B, 4) and ch <= H and cw <= W and mean.shape in ((C,), (C, H, W))
    out = np.empty((B, C, ch, cw), F)
    with np.errstate(all="ignore"):
        for i in range(B):
            yo, xo, m = min(int(plan[i, 0]), H - ch), min(int(plan[i, 1]), W - cw), plan[i, 2] != 0
            sy = yo + np.arange(ch)
            sx = xo + (cw - 1 - np.arange(cw) if m else np.arange(cw))
            v = chw[i][:, sy][:, :, sx].astype(F)
            mu = mean.reshape(C, 1, 1) if mean.ndim == 1 else mean[:, sy][:, :, sx]
            d = (v - mu).astype(F)
            out[i] = (d * scale).astype(F)
    return out


def same_bits(got, want):
    return V.same_bits(np.asarray(got, F), np.asarray(want, F))


# ---- the cases of the bare function
SCALES = (1.0, 1.0 / 256, 0.017, -1.0, 0.0)
# means: -0, a NaN, +-Inf, values that make v - mu round (v <= 255 is exact in 8 bits; 0.1 and 104.00001 are not), Caffe's usual three
MEAN_SPECIALS = (-0.0, float("nan"), float("inf"), float("-inf"), 0.1, 104.00001, 104.0, 117.0, 123.0, 0.0, -3.5, 1e-30)
CORNERS = (dict(chan=1, cw=1, ch=1, dw=0, dh=0, B=1),     # one output element in all
           dict(chan=3, cw=5, ch=3, dw=1, dh=2, B=3),     # 135 elements: the last thread owns three, every thread straddles rows
           dict(chan=4, cw=65, ch=3, dw=6, dh=2, B=5))    # 3900 elements: four workgroups, image and plane boundaries inside a thread's four


def function_cases(n=60, seed=21):
    """The corners under both layouts and both mean forms, then a seeded choice from the product chan x cw x ch x (W - cw) x (H - ch) x B x layout x mean form, about n
    in all -> [dict(chan, cw, ch, dw, dh, B, layout, pel, scale, k)]."""
    forms = list(itertools.product(("hwc", "chw"), (0, 1)))
    out = [dict(c, layout=l, pel=p) for c in CORNERS for l, p in forms]
    prod = list(itertools.product((1, 3, 4), (1, 5, 63, 64, 65), (1, 3), (0, 1, 6), (0, 2), (1, 3, 5), ("hwc", "chw"), (0, 1)))
    rng = np.random.default_rng(seed)
    for j in rng.choice(len(prod), n - len(out), replace=False):
        chan, cw, ch, dw, dh, B, l, p = prod[int(j)]
        out.append(dict(chan=chan, cw=cw, ch=ch, dw=dw, dh=dh, B=B, layout=l, pel=p))
    for k, c in enumerate(out):
        c["scale"] = SCALES[k % len(SCALES)]; c["k"] = k
    return out


def case_id(c):
    return f"{c['k']}-{c['layout']}-{'pel' if c['pel'] else 'chan'}-c{c['chan']}-{c['ch']}x{c['cw']}+{c['dh']}x{c['dw']}-b{c['B']}"


def plan_rows(ry, rx):
    """Offsets range over 0 .. ry / 0 .. rx.  All four corners with and without mirror; the mirror words 2 and 0x80000000, which must mirror; the offsets 0xFFFFFFFF
    and range + 1, which must clamp; word 3 is garbage throughout."""
    rows = [(y, x, m) for y in (0, ry) for x in (0, rx) for m in (0, 1)]
    rows += [(ry // 2, rx // 2, 2), (0, rx, 0x80000000), (0xFFFFFFFF, 0xFFFFFFFF, 0), (ry + 1, rx + 1, 1)]
    return [(y, x, m, GARBAGE ^ i) for i, (y, x, m) in enumerate(rows)]


def case_data(c):
    """-> (src dims, mean dims, src, mean, [plan per step]): src cycles through every byte value, the mean holds MEAN_SPECIALS (rotated by the case's index), and the
    steps deal plan_rows over the B images, other rows per image."""
    C, B = c["chan"], c["B"]
    H, W = c["ch"] + c["dh"], c["cw"] + c["dw"]
    rng = np.random.default_rng([c["k"], 5])
    n = B * C * H * W
    src = ((np.arange(n) * 37 + int(rng.integers(0, 256))) % 256).astype(U8)     # (37 is odd: a run of 256 holds every byte value)
    if c["layout"] == "hwc":
        sd = Dims.make("uint8_t", img=B, y=H, x=W, chan=C); src = src.reshape(B, H, W, C)
    else:
        sd = Dims.make("uint8_t", img=B, chan=C, y=H, x=W); src = src.reshape(B, C, H, W)
    sp = [MEAN_SPECIALS[(c["k"] + j) % len(MEAN_SPECIALS)] for j in range(len(MEAN_SPECIALS))]
    if c["pel"]:
        md = Dims.make("float", chan=C, y=H, x=W)
        mean = rng.uniform(0, 255, (C, H, W)).astype(F)
        flat = mean.reshape(-1); flat[::5] = np.array(sp, F)[np.arange(len(flat[::5])) % len(sp)]
    else:
        md = Dims.make("float", chan=C); mean = np.array(sp[:C], F)
    rows = plan_rows(c["dh"], c["dw"])
    steps = -(-len(rows) // B)
    plans = [np.array([rows[(s * B + i) % len(rows)] for i in range(B)], U32) for s in range(steps)]
    return sd, md, src, mean, plans


def run_steps(rtc, name, fop, vals, steps, keep=None, var_dims=None, bind=None):
    """eval_ref.run_steps for typed vars of any of the three types.  var_dims {arg: Dims}: the var's dims where they are not the op's; bind {arg: other arg}: bind
    the arg to the other arg's var."""
    spec = [(an, io) for an, io in pipe_func_args(fop)]
    var_dims = var_dims or {}; bind = bind or {}
    dims_of = lambda an: var_dims.get(an, fop.get_dims(an))
    rtc.compile([RtcFuncInfo(name, "", [a for a, _ in spec], fop)])
    made, am = [], {}
    guard = np.full(4, GUARD_BITS, U32).view(F)
    up = lambda an, a: rtc.copy_nda_to_var(f"{name}_{an}", np.ascontiguousarray(a, NP_OF[dims_of(an).tn]).reshape(dims_of(an).sizes))
    try:
        for an, _ in spec:
            if an in bind:
                continue
            vn = f"{name}_{an}"
            rtc.create_var_with_dims(vn, dims_of(an)); made.append(vn); am[an] = RtcArg.var(vn)
            rtc.create_var_with_dims(vn + "_guard", Dims.make("float", v=4)); made.append(vn + "_guard")
            rtc.copy_nda_to_var(vn + "_guard", guard)
        for an, other in bind.items():
            am[an] = am[other]
        for an, a in vals.items():
            up(an, a)
        call = RtcFuncCall(name, am)
        seen = []
        for st in steps:
            for an, a in st.items():
                up(an, a)
            rtc.run(call); rtc.finish_and_sync()
            if keep is not None:
                keep.append(rtc.last_launch() if rtc.be == "hip" else {})
            seen.append({an: rtc.copy_var_to_nda(f"{name}_{an}") for an, _ in spec if an not in bind})
        gv = {vn: rtc.copy_var_to_nda(vn) for vn in made if vn.endswith("_guard")}
        return seen, gv
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func(name); rtc.release_per_call_id_data()


def nan_out(shape):
    return np.full(shape, GUARD_BITS, U32).view(F)


def check_case(rtc, c, keep=None):
    sd, md, src, mean, plans = case_data(c)
    crop = (c["ch"], c["cw"])
    fop = data_transform_func_op(sd, crop, md, c["scale"])
    od = fop.get_dims("out")
    steps = [{"plan": p, "out": nan_out(od.sizes)} for p in plans]     # out pre-filled with NaN bits before every call
    seen, gv = run_steps(rtc, "dxf", fop, {"src": src, "mean": mean}, steps, keep=keep)
    for p, s in zip(plans, seen):
        want = data_transform_np(src, p, mean, c["scale"], crop, c["layout"])
        assert s["out"].dtype == F and s["out"].shape == want.shape
        assert same_bits(s["out"], want), (case_id(c), p.tolist())
        assert np.array_equal(np.isnan(s["out"]), np.isnan(want))
        assert s["src"].tobytes() == src.tobytes() and s["plan"].tobytes() == p.tobytes() and s["mean"].tobytes() == mean.tobytes(), "an input was written"
    E.guards_intact(gv, 4)
    return od.dims_prod()


def check_realistic(rtc, keep=None):
    """2 images 256 x 256 x 3 -> 227, mean_value (104, 117, 123), mirror on the second image."""
    rng = np.random.default_rng(99)
    src = rng.integers(0, 256, (2, 256, 256, 3)).astype(U8)
    src.reshape(-1)[:256] = np.arange(256, dtype=U8)     # every byte value
    mean = np.array([104, 117, 123], F)
    plan = np.array([[3, 29, 0, 0], [29, 0, 1, 0]], U32)
    fop = data_transform_func_op(Dims.make("uint8_t", img=2, y=256, x=256, chan=3), (227, 227), Dims.make("float", chan=3), 1.0)
    (s,), gv = run_steps(rtc, "dxr", fop, {"src": src, "mean": mean, "plan": plan, "out": nan_out((2, 3, 227, 227))}, [{}], keep=keep)
    want = data_transform_np(src, plan, mean, 1.0, (227, 227), "hwc")
    assert s["out"].tobytes() == want.tobytes()
    assert want[1, 2, 0, 0] == F(src[1, 29, 226, 2]) - F(123) and want[0, 0, 226, 226] == F(src[0, 3 + 226, 29 + 226, 0]) - F(104)
    E.guards_intact(gv, 4)


# ---- the refusals of the function, each with its sentence
def _op(src, plan, mean, out, scale=0.5, type_="DataTransform"):
    v = {"src": Nda(dims=src, tn=src.tn), "plan": Nda(dims=plan, tn=plan.tn), "mean": Nda(dims=mean, tn=mean.tn), "out": Nda(dims=out, tn=out.tn)}
    if scale is not None:
        v["scale"] = Nda(None, "float", (float(F(scale)),))
    return Op({"type": type_, "func_name": "hip_data_transform"}, v)


_S = Dims.make("uint8_t", img=2, y=5, x=6, chan=3)
_P = Dims.make("uint32_t", img=2, v=4)
_M = Dims.make("float", chan=3)
_O = Dims.make("float", img=2, chan=3, y=4, x=4)
BAD_OPS = [     # (what, the op, the exception, the sentence)
    ("src of type float", _op(Dims.make("float", img=2, y=5, x=6, chan=3), _P, _M, _O), RtErr, "src must be uint8_t img:y:x:chan or img:chan:y:x"),
    ("src with other dim names", _op(Dims.make("uint8_t", img=2, x=5, y=6, chan=3), _P, _M, _O), RtErr, "src must be uint8_t img:y:x:chan or img:chan:y:x"),
    ("out of type uint8_t", _op(_S, _P, _M, Dims.make("uint8_t", img=2, chan=3, y=4, x=4)), RtErr, "out must be float img:chan:y:x"),
    ("out channels-last", _op(_S, _P, _M, Dims.make("float", img=2, y=4, x=4, chan=3)), RtErr, "out must be float img:chan:y:x"),
    ("chan differs", _op(_S, _P, _M, Dims.make("float", img=2, chan=4, y=4, x=4)), RtErr, "out has chan=4, src chan=3"),
    ("images differ", _op(_S, _P, _M, Dims.make("float", img=3, chan=3, y=4, x=4)), RtErr, "out has 3 images, src 2"),
    ("crop taller than the source", _op(_S, _P, _M, Dims.make("float", img=2, chan=3, y=6, x=4)), RtErr, "the crop 6 x 4 is larger than the source 5 x 6"),
    ("crop wider than the source", _op(_S, _P, _M, Dims.make("float", img=2, chan=3, y=4, x=7)), RtErr, "the crop 4 x 7 is larger than the source 5 x 6"),
    ("mean at the crop size", _op(_S, _P, Dims.make("float", chan=3, y=4, x=4), _O), RtErr, r"mean must be float chan=3 or chan=3:y=5:x=6 \(the SOURCE size\)"),
    ("mean of one value", _op(_S, _P, Dims.make("float", chan=1), _O), RtErr, "mean must be float chan=3 or chan=3:y=5:x=6"),
    ("mean of another type", _op(_S, _P, Dims.make("uint32_t", chan=3), _O), RtErr, "mean must be float chan=3 or chan=3:y=5:x=6"),
    ("plan of type float", _op(_S, Dims.make("float", img=2, v=4), _M, _O), RtErr, r"plan must be uint32_t img=2:v=4"),
    ("plan of three words", _op(_S, Dims.make("uint32_t", img=2, v=3), _M, _O), RtErr, r"plan must be uint32_t img=2:v=4"),
    ("plan of another image count", _op(_S, Dims.make("uint32_t", img=3, v=4), _M, _O), RtErr, r"plan must be uint32_t img=2:v=4"),
    ("an op without scale", _op(_S, _P, _M, _O, scale=None), RtErr, "the op has no 'scale'"),
    ("an op without plan", Op({"type": "DataTransform", "func_name": "hip_data_transform"}, {"src": Nda(dims=_S, tn="uint8_t"), "mean": Nda(dims=_M, tn="float"), "out": Nda(dims=_O, tn="float"),
                                                                                              "scale": Nda(None, "float", (1.0,))}), RtErr, "the op has no 'plan'"),
    ("a source of 2 GiB", _op(Dims.make("uint8_t", img=2, y=32768, x=32768, chan=1), _P, Dims.make("float", chan=1), Dims.make("float", img=2, chan=1, y=4, x=4)), UnsupErr, "tensors of 2 GiB or more"),
    ("an out of 2 GiB", _op(Dims.make("uint8_t", img=2, y=16384, x=16384, chan=1), _P, Dims.make("float", chan=1), Dims.make("float", img=2, chan=1, y=16384, x=16384)), UnsupErr, "tensors of 2 GiB or more"),
    ("another op type", _op(_S, _P, _M, _O, type_="Accuracy"), RtErr, "a function of op type DataTransform, not Accuracy"),
]


def check_bad_ops(rtc):
    """Every op-level refusal, by the backend at compile and by the Python mirror (Op.data_geom) with the same sentence."""
    for what, op, exc, msg in BAD_OPS:
        with pytest.raises(exc, match=msg):
            rtc.compile([RtcFuncInfo("dxbad", "", ["src", "plan", "mean", "out"], op)])
        if op.get_type() == "DataTransform":
            with pytest.raises(exc, match=msg):
                op.data_geom()
    f = _op(_S, _P, _M, _O); f.nda_vals["img_shards"] = Nda(None, "uint32_t", (1,))
    with pytest.raises(RtErr, match="img_shards=1 on 'hip_data_transform': only hip_bconv_filts"):
        rtc.compile([RtcFuncInfo("dxbad", "", ["src", "plan", "mean", "out"], f)])


def check_bad_calls(rtc):
    """The refusals that need the call's vars: two args one var, vars whose image counts differ, a var of another type or other dims; then B-image ops on vars of B + 1
    images throughout, which run (the function is independent per image)."""
    sd, md = Dims.make("uint8_t", img=2, chan=1, y=2, x=2), Dims.make("float", chan=1, y=2, x=2)
    fop = data_transform_func_op(sd, (2, 2), md, 1.0)
    for a, b in (("src", "plan"), ("src", "mean"), ("src", "out"), ("plan", "mean"), ("plan", "out"), ("mean", "out")):     # (the alias is refused before types and dims)
        with pytest.raises(RtErr, match=f"args '{a}' and '{b}' are the same var 'dxa_{a}'"):
            run_steps(rtc, "dxa", fop, {}, [{}], bind={b: a})
    with pytest.raises(RtErr, match="arg 'plan' has 3 images, another arg 2"):
        run_steps(rtc, "dxa", fop, {}, [{}], var_dims={"plan": Dims.make("uint32_t", img=3, v=4)})
    with pytest.raises(RtErr, match="arg 'out' has 3 images, another arg 2"):
        run_steps(rtc, "dxa", fop, {}, [{}], var_dims={"out": Dims.make("float", img=3, chan=1, y=2, x=2)})
    with pytest.raises(RtErr, match=r"arg 'src' \(var 'dxa_src'\) has type float, the op says uint8_t"):
        run_steps(rtc, "dxa", fop, {}, [{}], var_dims={"src": Dims.make("float", img=2, chan=1, y=2, x=2)})
    with pytest.raises(RtErr, match="arg 'mean' has dims"):
        run_steps(rtc, "dxa", fop, {}, [{}], var_dims={"mean": Dims.make("float", chan=2, y=2, x=2)})
    with pytest.raises(RtErr, match="arg 'out' has dims"):
        run_steps(rtc, "dxa", fop, {}, [{}], var_dims={"out": Dims.make("float", img=2, chan=1, y=2, x=1)})
    # a B-image op on vars of B + 1 images
    c = dict(CORNERS[1], layout="hwc", pel=1, scale=0.017, k=3)
    sd, md, src, mean, _ = case_data(dict(c, B=c["B"] + 1))
    B1 = c["B"] + 1
    fop = data_transform_func_op(Dims(sd.names, (c["B"],) + sd.sizes[1:], "uint8_t"), (c["ch"], c["cw"]), md, c["scale"])
    plan = np.array([plan_rows(c["dh"], c["dw"])[i + 3] for i in range(B1)], U32)
    od = Dims.make("float", img=B1, chan=c["chan"], y=c["ch"], x=c["cw"])
    (s,), gv = run_steps(rtc, "dxb", fop, {"src": src, "mean": mean, "plan": plan, "out": nan_out(od.sizes)}, [{}],
                         var_dims={"src": sd, "plan": Dims.make("uint32_t", img=B1, v=4), "out": od})
    assert same_bits(s["out"], data_transform_np(src, plan, mean, c["scale"], (c["ch"], c["cw"]), "hwc"))
    E.guards_intact(gv, 4)


# ---- the drivers
SRC_MARGIN = {"chain": (3, 4), "residual": (2, 3)}     # the source is a few pels larger than `data`: (H - ch, W - cw)
XF_SOLVER = dict(type="adam", lr=0.01, momentum=0.9, weight_decay=5e-4, clip_gradients=1.0)


def make_pipe(name):
    if name == "residual":
        cp = bn_ref.residual(); return cp, add_bck_ops(cp), bn_ref.res_params(cp)
    mk, tops, seed = PIPES[name]
    cp = mk(); return cp, add_bck_ops(cp, loss_tops=tops), small_params(cp, seed)


def make_transform(name, seed=7):
    """chain: interleaved bytes, per-channel mean values, scale 1 / 256; residual: planar bytes, a per-pel mean, scale 1 / 64.  Both mirror."""
    cp = make_pipe(name)[0]
    d = cp.nodes["data"]
    assert d.dsz("y") == d.dsz("x")
    H, W = d.dsz("y") + SRC_MARGIN[name][0], d.dsz("x") + SRC_MARGIN[name][1]
    if name == "residual":
        mean = np.random.default_rng(5).uniform(90, 140, (d.dsz("chan"), H, W)).astype(F)
        return InputTransform((H, W), crop=d.dsz("y"), mirror=True, scale=1.0 / 64, mean=mean, layout="chw", seed=seed)
    return InputTransform((H, W), crop=d.dsz("y"), mirror=True, scale=1.0 / 256, mean_value=(104.0, 117.0, 123.0), layout="hwc", seed=seed)


def raw_inputs(xf, cp, k):
    """Pass k's bytes and labels."""
    d = cp.nodes["data"]
    rng = np.random.default_rng([k, 77])
    raw = rng.integers(0, 256, xf.src_dims(d.dsz("img"), d.dsz("chan")).sizes).astype(U8)
    n_class = bn_ref.N_CLASS if cp.name == "residual" else N_CLASS
    return raw, rng.integers(0, n_class, (d.dsz("img"), 1, 1)).astype(F)


def twin_of(xf, cp, raw, plan):
    return data_transform_np(raw, plan, xf.mean_array(cp.nodes["data"].dsz("chan")), xf.scale, (xf.ch, xf.cw), xf.layout)


def new_driver(rtc, name, xf=None, iter_size=1, solver=True, **kw):
    cp, bp, params = make_pipe(name)
    drv = ConvPipeBck(rtc, solver=Solver(**XF_SOLVER) if solver else None, iter_size=iter_size, input_transform=xf, **kw)
    drv.init(bp, params)
    return drv, bp


def all_vars(rtc, drv, skip=()):
    return {vn: rtc.copy_var_to_nda(vn).tobytes() for vn in drv.vars if vn not in skip}


XF_VARS = (DATA_RAW_VAR, DATA_XF_PLAN_VAR, DATA_XF_MEAN_VAR)


def check_step(rtc, name, iter_size=1, graph=None, passes=3, ref_rtc=None):
    """`passes` passes of adam with clipping on a driver WITH the transform fed bytes -- eager, or (graph = "serial" | "parallel") as replays of one captured graph --
    against an eager driver WITHOUT it fed the twin's floats under the same seeds: after each pass `data` is the twin under plan("train", k * B, B), and every var of
    the plain driver holds the same bytes in both."""
    ref_rtc = ref_rtc or rtc
    xf = make_transform(name)
    seed_var = graph is not None
    plain, bp = new_driver(ref_rtc, name, None, iter_size, seed_in_var=seed_var)
    want = []
    try:
        B = bp.nodes["data"].dsz("img")
        for k in range(passes):
            raw, label = raw_inputs(xf, bp.cp, k)
            data = twin_of(xf, bp.cp, raw, xf.plan("train", k * B, B))
            plain.set_det_drop_seed(1000 + k)
            plain.run_bck(["data", "label"], {"data": data, "label": label}, [])
            want.append((data, all_vars(ref_rtc, plain)))
    finally:
        plain.release()
    drv, bp = new_driver(rtc, name, xf, iter_size, seed_in_var=seed_var)
    try:
        assert [t for t, _, _ in drv.calls()][0] == DATA_XF_TAG and [t for t, _, _ in drv.calls()].count(DATA_XF_TAG) == 1
        assert drv.calls()[0][1].get_func_name() == "hip_data_transform" and set(XF_VARS) <= set(drv.vars)
        if graph is not None:
            assert drv.capture_graph(parallel=(graph == "parallel")) == len(drv.calls())
        for k in range(passes):
            raw, label = raw_inputs(xf, bp.cp, k)
            drv.set_det_drop_seed(1000 + k)
            assert drv.xf_images == k * B
            drv.run_bck([DATA_RAW_VAR, "label"], {DATA_RAW_VAR: raw, "label": label}, [], graph=graph is not None)
            assert np.array_equal(rtc.copy_var_to_nda(DATA_XF_PLAN_VAR), xf.plan("train", k * B, B)), (k, "the uploaded plan")
            assert rtc.copy_var_to_nda("data").tobytes() == want[k][0].tobytes(), (name, k, "data is not the twin's")
            got = all_vars(rtc, drv, XF_VARS)
            assert set(got) == set(want[k][1])
            for vn, b in want[k][1].items():
                assert got[vn] == b, (name, iter_size, graph, k, vn, "differs from the driver fed the twin's floats")
        assert drv.xf_images == passes * B
    finally:
        drv.release()


def check_call_deps(rtc, name):
    """The data_xf call is call 0, it depends on nothing, and every call that reads `data` has it among its dependencies."""
    drv, bp = new_driver(rtc, name, make_transform(name), seed_in_var=True)
    try:
        deps = drv._call_deps()
        assert deps[0] == []
        readers = [i for i, c in enumerate(drv.bck_calls) if i and any(io in ("IN", "INOUT") and c.rfc.arg_map[an].n == "data" for an, io in pipe_func_args(c.fop))]
        assert len(readers) >= 2     # (the first convolution and its filter gradient)
        for i in readers:
            assert 0 in deps[i], (i, drv.bck_calls[i].tag, deps[i])
    finally:
        drv.release()


def eval_raw_feed(xf, cp, k):
    raw, label = raw_inputs(xf, cp, 500 + k)
    return {DATA_RAW_VAR: raw, "label": label}


def check_eval(rtc, name, graph=False):
    """EvalPipe on a transforming driver: `data` is the twin under the centre plan; result() is the result of a driver without the transform fed the twin's floats."""
    xf = make_transform(name)
    drv, bp = new_driver(rtc, name, xf, seed_in_var=graph)
    try:
        B = bp.nodes["data"].dsz("img")
        ev = EvalPipe(drv, top_k=2)
        assert ev.calls()[0][0] == DATA_XF_TAG and ev.eval_calls[0].rfc is drv.bck_calls[0].rfc     # the driver's own call, reused
        if graph:
            assert ev.capture_graph() == len(ev.calls())
        centre = xf.plan("test", 0, B)
        assert centre.tolist() == [[SRC_MARGIN[name][0] // 2, SRC_MARGIN[name][1] // 2, 0, 0]] * B
        ev.reset()
        floats = []
        for k in range(2):
            fd = eval_raw_feed(xf, bp.cp, k)
            ev.run_batch(fd, graph=graph)
            floats.append(twin_of(xf, bp.cp, fd[DATA_RAW_VAR], centre))
            assert rtc.copy_var_to_nda("data").tobytes() == floats[k].tobytes(), (k, "data under the centre plan")
            assert np.array_equal(rtc.copy_var_to_nda(DATA_XF_PLAN_VAR), centre)
        got = ev.result()
        assert drv.xf_images == 0
        with pytest.raises(RtErr, match="feed 'data_raw'"):
            ev.run_batch({"data": floats[0], "label": fd["label"]})
        ev.release()
    finally:
        drv.release()
    plain, bp = new_driver(rtc, name, None)
    try:
        ev = EvalPipe(plain, top_k=2)
        want = ev.evaluate(2, lambda k: {"data": floats[k], "label": eval_raw_feed(xf, bp.cp, k)["label"]})
        ev.release()
    finally:
        plain.release()
    assert got == want and got["batches"] == 2, (got, want)


def xf_training_run(rtc, name, with_eval, graph=False):
    xf = make_transform(name)
    drv, bp = new_driver(rtc, name, xf, iter_size=2, seed_in_var=True)
    try:
        B = bp.nodes["data"].dsz("img")
        ev = EvalPipe(drv, top_k=2) if with_eval else None
        if graph:
            assert drv.capture_graph() == len(drv.calls())
            if ev is not None:
                assert ev.capture_graph() == len(ev.calls())
        for k in range(4):
            if ev is not None and k:
                n = drv.xf_images
                r = ev.evaluate(2, lambda i: eval_raw_feed(xf, bp.cp, 10 * k + i), graph=graph)
                assert r["batches"] == 2 and drv.xf_images == n
            raw, label = raw_inputs(xf, bp.cp, k)
            drv.set_det_drop_seed(1000 + k)
            drv.run_bck([DATA_RAW_VAR, "label"], {DATA_RAW_VAR: raw, "label": label}, [], graph=graph)
        assert drv.xf_images == 4 * B and (drv.iter, drv.micro) == (2, 0)
        return all_vars(rtc, drv)
    finally:
        if ev is not None:
            ev.release()
        drv.release()


def check_training_is_undisturbed(rtc, name, graph=False):
    """Four passes (iter_size=2) with a two-batch evaluation between every pair leave every driver var -- data_xf_plan included -- as the run without them."""
    plain = xf_training_run(rtc, name, False)
    mixed = xf_training_run(rtc, name, True, graph=graph)
    assert set(plain) == set(mixed)
    for vn in plain:
        assert plain[vn] == mixed[vn], (name, vn, "differs from the run without evaluations")


def calls_key(drv):
    return [(t, f.to_str(), sorted((an, a.n, None if a.v is None else a.v.tolist()) for an, a in am.items())) for t, f, am in drv.calls()]


def check_refusals_and_defaults(rtc):
    cp, bp, params = make_pipe("chain")
    a = ConvPipeBck(rtc); a.init(bp, params)
    try:
        base = (calls_key(a), list(a.vars))
    finally:
        a.release()
    b = ConvPipeBck(rtc, input_transform=None); b.init(bp, params)
    try:
        assert (calls_key(b), list(b.vars)) == base     # None leaves the call list and the vars as they are
        with pytest.raises(RtErr, match="built without an input_transform"):
            b.set_input_plan(np.zeros((2, 4), U32))
    finally:
        b.release()
    with pytest.raises(RtErr, match="input_transform must be an input_pipe.InputTransform"):
        ConvPipeBck(rtc, input_transform="caffe")
    xf = make_transform("chain")
    drv, bp = new_driver(rtc, "chain", xf, solver=False)
    try:
        assert calls_key(drv)[1:] == [(t, s, am) for t, s, am in base[0]] and [v for v in drv.vars if v not in XF_VARS] == base[1]
        raw, label = raw_inputs(xf, bp.cp, 0)
        data = twin_of(xf, bp.cp, raw, xf.plan("train", 0, 2))
        with pytest.raises(RtErr, match="would overwrite what is fed; feed 'data_raw'"):
            drv.run_bck(["data", "label"], {"data": data, "label": label}, [])
        assert drv.xf_images == 0
        # a caller's plan serves one pass; a bad one is refused before it is uploaded
        mine = np.array([[0, 4, 1, 9], [3, 0, 0, 9]], U32)
        drv.set_input_plan(mine)
        drv.run_bck([DATA_RAW_VAR, "label"], {DATA_RAW_VAR: raw, "label": label}, [])
        assert rtc.copy_var_to_nda("data").tobytes() == twin_of(xf, bp.cp, raw, mine).tobytes() and drv.xf_images == 2
        drv.run_bck([DATA_RAW_VAR, "label"], {DATA_RAW_VAR: raw, "label": label}, [])
        assert rtc.copy_var_to_nda("data").tobytes() == twin_of(xf, bp.cp, raw, xf.plan("train", 2, 2)).tobytes()
        with pytest.raises(RtErr, match=r"image 1: x_off=5 is beyond the range 0 \.\. 4"):
            drv.set_input_plan(np.array([[0, 0, 0, 0], [0, 5, 0, 0]], U32))
        # set_input_mean uploads the mean again
        drv.set_input_mean(np.array([1.0, 2.0, 3.0], F))
        drv.run_bck([DATA_RAW_VAR, "label"], {DATA_RAW_VAR: raw, "label": label}, [])
        want = data_transform_np(raw, xf.plan("train", 4, 2), np.array([1, 2, 3], F), xf.scale, (xf.ch, xf.cw), xf.layout)
        assert rtc.copy_var_to_nda("data").tobytes() == want.tobytes()
    finally:
        drv.release()
    # a data node of another crop; a node with one of the three names: both before anything is created
    for bad, msg in ((InputTransform((16, 17), crop=12), "must be float img:chan:y=12:x=12"), (InputTransform((16, 17)), "must be float img:chan:y=16:x=17")):
        d = ConvPipeBck(rtc, input_transform=bad)
        with pytest.raises(RtErr, match=msg):
            d.init(bp, params)
        assert d.vars == [] and d.bck_calls == []
    p = ConvPipe("clash", "data", Dims.make("float", img=2, chan=3, y=13, x=13))
    _conv(p, DATA_RAW_VAR, "data", 8, 3, 2)
    p.add(PipeOp("fc", "Convolution", DATA_RAW_VAR, "fc", out_chans=N_CLASS, kern_sz=(0, 0)))
    d = ConvPipeBck(rtc, input_transform=xf)
    with pytest.raises(RtErr, match="needs the var name 'data_raw', which is a node of the pipe"):
        d.init(add_bck_ops(p), None)
    assert d.vars == []
    with pytest.raises(RtErr, match="3 mean values|2 mean values"):
        d2 = ConvPipeBck(rtc, input_transform=InputTransform((16, 17), crop=13, mean_value=(1.0, 2.0)))
        d2.init(bp, params)
