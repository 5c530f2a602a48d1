"""What tests/test_resnet_pipe_cpu.py and tests/test_gpu_resnet.py share: the shapes, the numpy restatement of hip_chan_affine and of the fp32 ResNet forward pass,
explicit He-scaled params, the function ops of the residual convolution's cases (also written to tests/golden/ops/resnet-ops.txt, which __graft_entry__.build()
pre-specialises) and the derived error bound of the residual epilogue."""
import numpy as np

from boda_amd import conv_pipe as cpm, nhwc
from boda_amd.cnn_op import OpTune, add_codegen_annotations, chan_affine_func_op
from boda_amd.cnn_op import NATIVE_ARGS
from boda_amd.op import Dims, parse_op
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo
from oracle import boda_oracle as bo

# hip_chan_affine: plane sizes 1, 3, 49, 64 (a lone element, a tail only, an odd plane, whole quads), 1 / 5 / 8 channels, 1 / 3 images
AFFINE_SHAPES = [(B, C, H, W) for (H, W) in ((1, 1), (1, 3), (7, 7), (8, 8)) for C in (1, 5, 8) for B in (1, 3)]


def affine_data(shape, seed=0):
    """in with both signs, exact zeros and a -0 among them; a with both signs; b of in's size, so that the ReLU cuts some sums."""
    rng = np.random.default_rng(seed + 7919 * int(np.prod(shape)))
    x = rng.uniform(-2, 2, shape).astype(np.float32)
    x.reshape(-1)[::5] = 0.0; x.reshape(-1)[0] = -0.0
    a = rng.uniform(-2, 2, shape[1]).astype(np.float32); b = rng.uniform(-1, 1, shape[1]).astype(np.float32)
    if shape[1] > 1:
        b[0] = 0.0      # (x = +-0 then gives a*x + 0 = +-0: the ReLU must make it +0)
    return x, a, b


def chan_affine_ref(x, a, b, relu):
    """out = in * a[chan] + b[chan]: an fp32 multiply, then an fp32 add (numpy fuses nothing); relu: x > 0 ? x : +0."""
    v = x.astype(np.float32) * a.astype(np.float32)[None, :, None, None]
    v = v + b.astype(np.float32)[None, :, None, None]
    if relu:
        v = np.where(v > 0, v, np.float32(0.0))
    return v.astype(np.float32)


def affine_op(shape, relu):
    return chan_affine_func_op(Dims.make("float", img=shape[0], chan=shape[1], y=shape[2], x=shape[3]), relu)


def bits_eq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_affine(rtc, shape, relu, in_place, x, a, b):
    """One hip_chan_affine call on `rtc` with host inputs, out of place or on the input var itself -> out."""
    f = affine_op(shape, relu)
    rtc.compile([RtcFuncInfo("f", "", [n for n, _ in NATIVE_ARGS["hip_chan_affine"]], f)])
    made = []
    try:
        for vn, an in (("x", "in"), ("a", "a"), ("b", "b")) + (() if in_place else (("y", "out"),)):
            rtc.create_var_with_dims(vn, f.get_dims(an)); made.append(vn)
        rtc.copy_nda_to_var("x", x); rtc.copy_nda_to_var("a", a); rtc.copy_nda_to_var("b", b)
        out = "x" if in_place else "y"
        rtc.run(RtcFuncCall("f", {"in": RtcArg.var("x"), "a": RtcArg.var("a"), "b": RtcArg.var("b"), "out": RtcArg.var(out)})); rtc.finish_and_sync()
        got = rtc.copy_var_to_nda(out)
        if not in_place:
            assert bits_eq(rtc.copy_var_to_nda("x"), x)     # the input is left alone
        return got
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


# ---- the residual convolution, one op at a time: 1x1 / stride 1 / unpadded, (B, C, HW, OC, forced tile)
RES_CASES = {
    "ragged_2x24x7x40": (2, 24, 7, 40, ""),             # ragged pel and out_chan tiles
    "scalar_1x16x5x36": (1, 16, 5, 36, ""),             # out_chans no multiple of 8: element stores (and 8-byte loads: 36 is a multiple of 4)
    "elemloads_1x16x5x38": (1, 16, 5, 38, ""),          # a row pitch that is no multiple of 4 channels: element loads of res as well (a case of this file's own)
    "blocks_2x64x14x256": (2, 64, 14, 256, ""),         # 28 workgroups
    "ksl4_2x512x7x64": (2, 512, 7, 64, "64x64x64x2x2x2x4"),   # a forced tile that carries 4 K slices: the last arriver runs the epilogue
}
NHWC = dict(hip_dtype="bf16", hip_layout="nhwc")


def conv_op(B, C, HW, OC, k=1, pad=0):
    return parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts=(dims=(out_chan={OC},in_chan={C},y={k},x={k})),"
                    f"in=(dims=(img={B},chan={C},y={HW},x={HW})),in_pad=(tn=none,dims=(y={pad},x={pad})),kern_sz=(tn=none,dims=(y={k},x={k})),"
                    f"out=(dims=(img={B},chan={OC},y={HW},x={HW})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y=1,x=1))))")


def res_func_op(case, out_f32, relu):
    """The flagged function op of one case: annotate, set conv_has_relu, nhwc.fuse_residual."""
    B, C, HW, OC, tile = RES_CASES[case]
    a = add_codegen_annotations(conv_op(B, C, HW, OC), OpTune(hip_out="f32" if out_f32 else "", hip_tile=tile, **NHWC))
    a.nda_vals["conv_has_relu"].v = (int(relu),)
    nhwc.fuse_residual(a)
    return a


def res_func_ops():
    return [res_func_op(c, o, r) for c in RES_CASES for o in (False, True) for r in (1, 0)]


def golden_lines():
    """tests/golden/ops/resnet-ops.txt: every function op the two test files run one at a time."""
    return [affine_op(s, r).to_str() for s in AFFINE_SHAPES for r in (0, 1)] + [a.to_str() for a in res_func_ops()]


def res_data(case, out_f32, seed=0):
    """res in the var's own layout (img:y:x:chan) and element type, both signs, of the convolution's own magnitude (so that the ReLU cuts some sums):
    -> (what is uploaded: float32, or the uint16 patterns of bf16; the same values as float32 img:chan:y:x)."""
    B, C, HW, OC, _ = RES_CASES[case]
    s = 8.0 * np.sqrt(C)     # (mode-5 operands are U(-5, 5): a sum of C products has a standard deviation of about 8.3 sqrt(C))
    r = bo.to_bf16(np.random.default_rng(seed + OC).uniform(-s, s, (B, HW, HW, OC)).astype(np.float32))     # (bf16 values for BOTH output types: one res for the two launches)
    up = r if out_f32 else (r.view(np.uint32) >> 16).astype(np.uint16)
    return np.ascontiguousarray(up), np.ascontiguousarray(r.transpose(0, 3, 1, 2))


def res_want_and_limit(inp, filts, biases, res, relu, stride=(1, 1), pad=(0, 0)):
    """want = relu(conv_fwd(bf16 in, bf16 filts, biases, no relu) + float(res)) from the oracle, and the derived bound of tests/test_gpu_nhwc.py with one more
    addition and S' = S + |res|:  |got - want| <= 2 (K + 2) 2^-24 S'  (kernel and oracle add the same exact products, the bias and res in different orders: K + 2
    fp32 additions, each order within (K + 2) u S' of the exact sum; the ReLU is 1-Lipschitz).  A bf16 output adds 2^-8 (|want| + that): bf16_limit()."""
    K = filts.shape[1] * filts.shape[2] * filts.shape[3]
    i16, f16 = bo.to_bf16(inp), bo.to_bf16(filts)
    want = bo.conv_fwd(i16, f16, biases, stride, pad, False)
    S = bo.conv_fwd(np.abs(i16), np.abs(f16), np.abs(biases), stride, pad, False).astype(np.float64)
    if res is not None:      # (res=None: a plain convolution -- the bound of tests/test_gpu_nhwc.py itself, K + 1 additions)
        want = want + res.astype(np.float32); S = S + np.abs(res.astype(np.float64))
    if relu:
        want = np.where(want > 0, want, np.float32(0.0)).astype(np.float32)
    return want.astype(np.float32), 2.0 * (K + (2 if res is not None else 1)) * 2.0 ** -24 * S


def bf16_limit(want, lim):
    return lim + 2.0 ** -8 * (np.abs(want.astype(np.float64)) + lim)


# ---- whole nets
def he_params(cp, seed=0):
    """Explicit params for every param of the pipe: He-scaled filters (std sqrt(2 / fan_in)), small biases, BatchNorm var in [0.5, 2] and mean in [-0.5, 0.5],
    Scale scale in [0.5, 1.5] and bias in [-0.2, 0.2] -- 50 layers stay finite."""
    rng = np.random.default_rng(seed)
    P = {}
    for pn, d in cp.params.items():
        if pn.endswith("_filts"):
            fan_in = d.dsz("in_chan") * d.dsz("y") * d.dsz("x")
            P[pn] = (rng.standard_normal(d.sizes) * np.sqrt(2.0 / fan_in)).astype(np.float32)
        elif pn.endswith("_biases"):
            P[pn] = rng.uniform(-0.1, 0.1, d.sizes).astype(np.float32)
        elif pn.endswith("_var"):
            P[pn] = rng.uniform(0.5, 2.0, d.sizes).astype(np.float32)
        elif pn.endswith("_mean"):
            P[pn] = rng.uniform(-0.5, 0.5, d.sizes).astype(np.float32)
        elif pn.endswith("_scale"):
            P[pn] = rng.uniform(0.5, 1.5, d.sizes).astype(np.float32)
        else:
            P[pn] = rng.uniform(-0.2, 0.2, d.sizes).astype(np.float32)
    return P


def truncated(cp, last_top):
    """The pipe up to and including the last op that writes `last_top`."""
    t = cpm.ConvPipe(cp.name, cp.in_node, cp.nodes[cp.in_node])
    n = max(i for i, o in enumerate(cp.ops) if o.top == last_top) + 1
    for o in cp.ops[:n]:
        t.add(cpm.PipeOp(o.tag, o.type, o.bot, o.top, out_chans=o.out_chans, kern_sz=o.kern_sz, stride=o.stride, in_pad=o.in_pad, avg_pool=o.avg_pool, lrn=o.lrn, bots=o.bots, eps=o.eps))
    return t


def run_steps(cp):
    """The pipe as the fp32 driver runs it: [(kind, ops)] with kind conv | affine | pool | eltwise | relu; an affine step is a whole run plus its ReLU."""
    steps, i, ops = [], 0, cp.ops
    while i < len(ops):
        o = ops[i]
        if o.type == "Convolution":
            relu = i + 1 < len(ops) and ops[i + 1].type == "ReLU" and ops[i + 1].bot == o.top
            steps.append(("conv", [o], relu)); i += 2 if relu else 1
        elif o.type in cpm.AFFINE_TYPES:
            j = i
            while j < len(ops) and ops[j].type in cpm.AFFINE_TYPES and ops[j].bot == o.bot:
                j += 1
            relu = j < len(ops) and ops[j].type == "ReLU" and ops[j].bot == o.bot
            steps.append(("affine", ops[i:j], relu)); i = j + (1 if relu else 0)
        elif o.type == "Pooling":
            steps.append(("pool", [o], False)); i += 1
        elif o.type == "Eltwise":
            steps.append(("eltwise", [o], False)); i += 1
        elif o.type == "ReLU":
            steps.append(("relu", [o], False)); i += 1
        else:
            raise AssertionError(o.type)
    return steps


def affine_steps(P, run):
    return [("BatchNorm", P[o.tag + "_mean"], P[o.tag + "_var"], o.eps) if o.type == "BatchNorm" else ("Scale", P[o.tag + "_scale"], P[o.tag + "_bias"]) for o in run]


def ref_forward_f32(cp, P, x):
    """Every node's value after each step, in numpy fp32: {(step index, node): array} and the final {node: array}.  Convolutions are bo.conv_fwd (the reference's fma
    chain), affine runs fold_affine + the written formula, Eltwise a chain from +0 in the order of bots, ReLU x > 0 ? x : +0."""
    val = {cp.in_node: x}
    snaps = []
    for kind, ops, relu in run_steps(cp):
        o = ops[0]
        if kind == "conv":
            val[o.top] = bo.conv_fwd(val[o.bot], P[o.tag + "_filts"], P[o.tag + "_biases"], tuple(o.stride), tuple(o.in_pad), bool(relu))
        elif kind == "affine":
            a, b = cpm.fold_affine(affine_steps(P, ops))
            val[o.top] = chan_affine_ref(val[o.bot], a, b, relu)
        elif kind == "pool":
            val[o.top] = bo.pool_fwd(val[o.bot], tuple(o.kern_sz), tuple(o.stride), tuple(o.in_pad), bool(o.avg_pool))
        elif kind == "eltwise":
            v = np.zeros_like(val[o.bots[0]])
            for b in o.bots:
                v = v + val[b]
            val[o.top] = v.astype(np.float32)
        else:
            v = val[o.bot]; val[o.top] = np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
        snaps.append((kind, o.top, val[o.top].copy()))
    return val, snaps
