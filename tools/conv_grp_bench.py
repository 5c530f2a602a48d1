"""Times the grouped convolution's three functions on be=hip (hip_conv_grp, hip_bconv_in_grp, hip_bconv_filts_grp; kernels/conv_grp_f32.hip), layer by layer: AlexNet
conv2 / conv4 / conv5 at 256 images, ResNeXt-50 32x4d's four 3x3 layer shapes at 32 images, MobileNet-v1's depthwise shapes at 32 images.  Not part of the suite.

    python tools/conv_grp_bench.py [--sets alexnet,resnext,mobilenet] [--runs 5] [--warmup 2] [--blocks 3] [--funcs fwd,in,filts] [--layers _s1] [--tile T]

Per layer and function one JSON line: the median us of the grouped call, its launch (kernel = the form, configuration = BK / KSL), TF/s of the flops the op counts
(2 B OC OH OW CG KH KW), GB/s of the call's algorithmic bytes beside the recorded 6.29 TB/s copy rate, and the yardstick measured IN THE SAME PROCESS in alternating
blocks (grouped, yardstick, grouped, ...): what a user can do without the grouped functions -- hip_split per group, the ungrouped function per group, hip_concat per
group (the filter gradient needs no concat: a group's rows are a tensor of their own) --, timed from its first call's start to its last call's end.  Depthwise sets
(hundreds of groups: slice-and-call is not usable) have the copy rate as their yardstick instead.  No figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boda_amd import gen_data as gd  # noqa: E402
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_codegen_annotations, add_pipe_op_annotations  # noqa: E402
from boda_amd.op import parse_op  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402

COPY_GBS = 6290.0   # the recorded device-to-device copy rate
SETS = {   # name -> [(layer, (B, g, C, OC, H, W, k, stride, pad))]
    "alexnet": [("conv2", (256, 2, 96, 256, 27, 27, 5, 1, 2)), ("conv4", (256, 2, 384, 384, 13, 13, 3, 1, 1)), ("conv5", (256, 2, 384, 256, 13, 13, 3, 1, 1))],
    "resnext": [(f"conv{i + 2}_3x3", (32, 32, c, c, hw, hw, 3, 1, 1)) for i, (c, hw) in enumerate(((128, 56), (256, 28), (512, 14), (1024, 7)))],
    "mobilenet": [(f"dw{c}_{hw}_s{s}", (32, c, c, c, hw, hw, 3, s, 1)) for c, hw, s in ((32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2),
                                                                                     (512, 14, 1), (512, 14, 2), (1024, 7, 1))],
}


def ops_of(B, g, C, OC, H, W, k, s, p, group=True):
    """-> (Convolution, BckConv) ops of a layer; group=False: ONE group's ungrouped slice."""
    if not group:
        C, OC, g = C // g, OC // g, 1
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    grp = f"group=(tn=uint32_t,v={g})," if g > 1 else ""
    f, i, o = f"(dims=(out_chan={OC},in_chan={C // g},y={k},x={k}))", f"(dims=(img={B},chan={C},y={H},x={W}))", f"(dims=(img={B},chan={OC},y={OH},x={OW}))"
    geo = f"in_pad=(tn=none,dims=(y={p},x={p})),kern_sz=(tn=none,dims=(y={k},x={k})),out_chans=(tn=uint32_t,v={OC}),stride=(tn=none,dims=(y={s},x={s}))"
    cv = parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={OC})),filts={f},{grp}in={i},out={o},{geo}))")
    bk = parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts={f},filts_grad_loss={f},{grp}in={i},in_grad_loss={i},"
                  f"out_grad_loss={o},{geo}))")
    return cv, bk


def plumbing(B, chans, H, W, typ):
    """The hip_split / hip_concat function ops of G equal channel ranges (one call per range)."""
    d = lambda c: f"(dims=(img={B},chan={c},y={H},x={W}))"
    if typ == "Split":
        op = parse_op(f"(str_vals=(type=Split),nda_vals=(in={d(sum(chans))}," + ",".join(f"outs_{i}={d(c)}" for i, c in enumerate(chans)) + f",outs_num=(tn=uint32_t,v={len(chans)})))")
    else:
        op = parse_op(f"(str_vals=(type=Concat),nda_vals=(" + ",".join(f"ins_{i}={d(c)}" for i, c in enumerate(chans)) + f",ins_num=(tn=uint32_t,v={len(chans)}),out={d(sum(chans))}))")
    return add_pipe_op_annotations(op, OpTune())


class Bench:
    def __init__(self, rtc):
        self.rtc, self.vars, self.funcs = rtc, [], []

    def var(self, vn, dims, gen=None):
        self.rtc.create_var_with_dims(vn, dims); self.vars.append(vn)
        if gen:
            self.rtc.run(gd.gen_call(gen[0], gen[1], vn, dims, 5, 0.0))
        return vn

    def func(self, name, fop, binds):
        """Compile one function op and -> its call, args bound to the vars `binds` names (REF args from the op)."""
        fn = fop.get_func_name()
        self.rtc.compile([RtcFuncInfo(name, "", [a for a, _ in NATIVE_ARGS[fn]], fop)]); self.funcs.append(name)
        return RtcFuncCall(name, {an: (RtcArg.ref(fop.get_dims(an)) if io == "REF" else RtcArg.var(binds[an])) for an, io in NATIVE_ARGS[fn]})

    def release(self):
        self.rtc.finish_and_sync()
        for vn in self.vars:
            self.rtc.release_var(vn)
        for fn in self.funcs:
            self.rtc.release_func(fn)
        self.rtc.release_per_call_id_data()


def bench_layer(rtc, case, which, runs, warmup, blocks, slice_and_call, tile=""):
    B, g, C, OC, H, W, k, s, p = case
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cv, bk = ops_of(*case)
    fi, _, ff = add_bck_conv_annotations(bk, OpTune())
    fop = {"fwd": add_codegen_annotations(cv, OpTune()), "in": fi, "filts": ff}[which]
    if tile:   # a seven-field tile forces the grouped call's form and blocking (the yardstick keeps the planner's)
        fop = fop.copy(); fop.str_vals["hip_tile"] = tile
    typ = "Convolution" if which == "fwd" else "BckConv"
    b = Bench(rtc)
    try:
        binds = {}
        for an, io in NATIVE_ARGS[fop.get_func_name()]:
            if io != "REF":
                binds[an] = b.var("g_" + an, fop.get_dims(an), (typ, an) if io == "IN" else None)
        grouped = [b.func("g_call", fop, binds)]
        yard = []
        if slice_and_call:   # split per group, the ungrouped function per group, concat per group -- on vars of their own
            scv, sbk = ops_of(*case, group=False)
            si, _, sf = add_bck_conv_annotations(sbk, OpTune())
            sfop = {"fwd": add_codegen_annotations(scv, OpTune()), "in": si, "filts": sf}[which]
            wide_in = {"fwd": ["in"], "in": ["out_grad_loss"], "filts": ["in", "out_grad_loss"]}[which]
            wide_out = {"fwd": "out", "in": "in_grad_loss", "filts": None}[which]
            plane = {"in": (C // g, H, W), "out_grad_loss": (OC // g, OH, OW), "out": (OC // g, OH, OW), "in_grad_loss": (C // g, H, W)}
            for an in wide_in:
                c, h, w = plane[an]
                for j, sp in enumerate(plumbing(B, [c] * g, h, w, "Split")):
                    v = b.var(f"y_{an}_{j}", sp.get_dims("out"))
                    yard.append(b.func(f"y_split_{an}_{j}", sp, {"in": binds[an], "out": v}))
            for j in range(g):
                sb = {}
                for an, io in NATIVE_ARGS[sfop.get_func_name()]:
                    if io == "REF":
                        continue
                    sb[an] = f"y_{an}_{j}" if an in wide_in else b.var(f"y_{an}_{j}", sfop.get_dims(an), (typ, an) if io == "IN" else None)
                yard.append(b.func(f"y_call_{j}", sfop, sb))
            if wide_out:
                c, h, w = plane[wide_out]
                wv = b.var("y_wide_out", fop.get_dims(wide_out))
                for j, cc in enumerate(plumbing(B, [c] * g, h, w, "Concat")):
                    yard.append(b.func(f"y_concat_{j}", cc, {"in": f"y_{wide_out}_{j}", "out": wv}))
        for calls in (grouped, yard):
            for _ in range(max(1, warmup)):
                for c in calls:
                    rtc.run(c)
            if calls is grouped:
                launch = rtc.last_launch()
        tg, ty = [], []
        for _ in range(blocks):
            for calls, acc in ((grouped, tg), (yard, ty)):
                if not calls:
                    continue
                ids = [[rtc.run(c) for c in calls] for _ in range(runs)]
                rtc.finish_and_sync()
                acc += [rtc.get_dur(i[0], i[-1]) * 1e3 for i in ids]
                rtc.release_per_call_id_data()
        us = statistics.median(tg)
        flops = cv.flops()
        nbytes = sum(fop.get_dims(an).bytes_sz() for an, io in NATIVE_ARGS[fop.get_func_name()] if io != "REF")
        row = {"func": fop.get_func_name(), "us": round(us, 1), "kernel": launch["kernel"], "cfg": launch["cfg"], "grid": launch["grid"], "tflops": round(flops / us / 1e6, 3),
               "gbs": round(nbytes / us / 1e3, 1), "frac_copy_rate": round(nbytes / us / 1e3 / COPY_GBS, 4)}
        if ty:
            row.update({"slice_and_call_us": round(statistics.median(ty), 1), "slice_and_call_launches": len(yard), "grouped_over_slice_and_call": round(us / statistics.median(ty), 3)})
        else:
            row["copy_rate_us"] = round(nbytes / COPY_GBS / 1e3, 1)
        return row
    finally:
        b.release()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sets", default="alexnet,resnext,mobilenet"); ap.add_argument("--funcs", default="fwd,in,filts")
    ap.add_argument("--tile", default="", help="a seven-field tile BIxBJxBKxWIxWJxMINWxKSL for the grouped call (use with one --funcs): a forced-form comparison run")
    ap.add_argument("--layers", default="", help="comma list: only the layers whose name contains one of these (e.g. _s1: the stride-1 depthwise shapes)")
    ap.add_argument("--runs", type=int, default=5); ap.add_argument("--warmup", type=int, default=2); ap.add_argument("--blocks", type=int, default=3)
    a = ap.parse_args()
    rtc = make_rtc("(be=hip)", 0); rtc.init()
    rtc.compile(gd.func_infos())
    try:
        for sn in a.sets.split(","):
            for layer, case in SETS[sn]:
                if a.layers and not any(x in layer for x in a.layers.split(",")):
                    continue
                for which in a.funcs.split(","):
                    row = bench_layer(rtc, case, which, a.runs, a.warmup, a.blocks, slice_and_call=(sn != "mobilenet"), tile=a.tile)
                    print(json.dumps(dict({"set": sn, "layer": layer, "case": list(case)}, **({"forced_tile": a.tile} if a.tile else {}), **row)), flush=True)
    finally:
        rtc.close()


if __name__ == "__main__":
    main()
