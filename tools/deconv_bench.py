"""Times the Deconvolution family's three functions on be=hip (hip_deconv, hip_deconv_bck_in, hip_deconv_bck_filts; kernels/deconv_f32.hip), layer by layer: FCN's three
upsampling heads at 8 images (21 -> 21 channels at 4/2 on 16 x 16, 16/8 on 34 x 34, 64/32 on 16 x 16) and a decoder layer (256 -> 128, 4/2 on 28 x 28 at 32 images).
Not part of the suite.

    python tools/deconv_bench.py [--sets fcn,decoder] [--runs 5] [--warmup 2] [--blocks 3] [--funcs fwd,in,filts] [--layers up2] [--tile T]

Per layer and function one JSON line: the path the planner takes for the layer (cnn_op.deconv_form), the median us of the direct call, its launch (configuration = BK / KSL), GB/s of the call's algorithmic bytes beside the recorded
6.29 TB/s copy rate, and the OTHER PATH measured in the same process in alternating blocks (direct, other, direct, ...) where it can run on the shape: the existing
matrix function on the exchanged roles -- hip_bconv_in (then hip_chan_affine for the bias) for the forward, hip_conv for the data gradient, hip_bconv_filts for the
filter gradient --, timed from its first call's start to its last call's end.  No figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boda_amd import gen_data as gd  # noqa: E402
from boda_amd.cnn_op import (NATIVE_ARGS, OpTune, add_bck_conv_annotations, add_bck_deconv_annotations, add_codegen_annotations, add_deconv_annotations,  # noqa: E402
                             chan_affine_func_op, deconv_form)
from boda_amd.op import parse_op  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402

COPY_GBS = 6290.0   # the recorded device-to-device copy rate
SETS = {   # name -> [(layer, (B, C, H, W, OC, k, stride, pad))]
    "fcn": [("up_4_2", (8, 21, 16, 16, 21, 4, 2, 0)), ("up_16_8", (8, 21, 34, 34, 21, 16, 8, 0)), ("up_64_32", (8, 21, 16, 16, 21, 64, 32, 0))],
    "decoder": [("dec_256_128", (32, 256, 28, 28, 128, 4, 2, 1))],
}


def ops_of(B, C, H, W, OC, k, s, p):
    """-> (Deconvolution, BckDeconv, the exchanged Convolution, the exchanged BckConv) ops of a layer."""
    OH, OW = (H - 1) * s + k - 2 * p, (W - 1) * s + k - 2 * p
    geo = lambda oc: f"in_pad=(tn=none,dims=(y={p},x={p})),kern_sz=(tn=none,dims=(y={k},x={k})),out_chans=(tn=uint32_t,v={oc}),stride=(tn=none,dims=(y={s},x={s}))"
    small, big = f"(dims=(img={B},chan={C},y={H},x={W}))", f"(dims=(img={B},chan={OC},y={OH},x={OW}))"
    f = f"(dims=(in_chan={C},out_chan={OC},y={k},x={k}))"
    dc = parse_op(f"(str_vals=(type=Deconvolution),nda_vals=(biases=(dims=(out_chan={OC})),filts={f},in={small},out={big},{geo(OC)}))")
    bd = parse_op(f"(str_vals=(type=BckDeconv),nda_vals=(biases=(dims=(out_chan={OC})),biases_grad_loss=(dims=(out_chan={OC})),filts={f},filts_grad_loss={f},in={small},"
                  f"in_grad_loss={small},out_grad_loss={big},{geo(OC)}))")
    xf = f"(dims=(out_chan={C},in_chan={OC},y={k},x={k}))"   # the same blob read as the filters of the convolution OC -> C
    xc = parse_op(f"(str_vals=(type=Convolution),nda_vals=(biases=(dims=(out_chan={C})),filts={xf},in={big},out={small},{geo(C)}))")
    xb = parse_op(f"(str_vals=(type=BckConv),nda_vals=(biases=(dims=(out_chan={C})),biases_grad_loss=(dims=(out_chan={C})),filts={xf},filts_grad_loss={xf},in={big},"
                  f"in_grad_loss={big},out_grad_loss={small},{geo(C)}))")
    return dc, bd, xc, xb


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

    def bound(self, name, fop, typ):
        """A function on vars of its own, the inputs filled with generated data."""
        binds = {}
        for an, io in NATIVE_ARGS[fop.get_func_name()]:
            if io != "REF":
                binds[an] = self.var(f"{name}_{an}", fop.get_dims(an), (typ, an) if io == "IN" else None)
        return self.func(name, fop, binds), binds

    def release(self):
        self.rtc.finish_and_sync()
        for vn in self.vars:
            self.rtc.release_var(vn)
        for fn in self.funcs:
            self.rtc.release_func(fn)
        self.rtc.release_per_call_id_data()


def bench_layer(rtc, case, which, runs, warmup, blocks, tile=""):
    dc, bd, xc, xb = ops_of(*case)
    fi, _, ff = add_bck_deconv_annotations(bd, OpTune(), form="direct")
    fop = {"fwd": add_deconv_annotations(dc, OpTune(), form="direct"), "in": fi, "filts": ff}[which]
    if tile:
        fop = fop.copy(); fop.str_vals["hip_tile"] = tile
    b = Bench(rtc)
    try:
        direct = [b.bound("d_call", fop, "Convolution" if which == "fwd" else "BckConv")[0]]
        other, why = [], ""
        try:   # the existing matrix function on the exchanged roles, where it takes the shape
            xi, _, xff = add_bck_conv_annotations(xb, OpTune())
            if which == "fwd":
                c, binds = b.bound("x_call", xi, "BckConv")
                aff = chan_affine_func_op(xi.get_dims("in_grad_loss"), 0)
                ones = b.var("x_ones", aff.get_dims("a"), ("Convolution", "biases")); bias = b.var("x_bias", aff.get_dims("b"), ("Convolution", "biases"))
                other = [c, b.func("x_affine", aff, {"in": binds["in_grad_loss"], "a": ones, "b": bias, "out": binds["in_grad_loss"]})]
            elif which == "in":
                xa = add_codegen_annotations(xc, OpTune()); del xa.nda_vals["conv_has_relu"]; xa.set_u32("conv_has_relu", 0)
                other = [b.bound("x_call", xa, "Convolution")[0]]
            else:
                other = [b.bound("x_call", xff, "BckConv")[0]]
        except Exception as e:   # (a geometry outside the existing function's limits: refused at compile)
            other, why = [], str(e)[:160]
        for _ in range(max(1, warmup)):
            rtc.run(direct[0])
        launch = rtc.last_launch()
        try:   # (some limits are the launch's, not the compile's)
            for _ in range(max(1, warmup) if other else 0):
                for c in other:
                    rtc.run(c)
        except Exception as e:
            other, why = [], str(e)[:160]
        td, to = [], []
        for _ in range(blocks):
            for calls, acc in ((direct, td), (other, to)):
                if not calls:
                    continue
                ids = [[rtc.run(c) for c in calls] for _ in range(runs)]
                rtc.finish_and_sync()
                acc += [rtc.get_dur(i[0], i[-1]) * 1e3 for i in ids]
                rtc.release_per_call_id_data()
        us = statistics.median(td)
        nbytes = sum(fop.get_dims(an).bytes_sz() for an, io in NATIVE_ARGS[fop.get_func_name()] if io != "REF")
        row = {"planner": deconv_form(dc, OpTune()), "func": fop.get_func_name(), "us": round(us, 1), "kernel": launch["kernel"], "cfg": launch["cfg"], "grid": launch["grid"], "tflops": round(dc.flops() / us / 1e6, 3),
               "gbs": round(nbytes / us / 1e3, 1), "frac_copy_rate": round(nbytes / us / 1e3 / COPY_GBS, 4), "copy_rate_us": round(nbytes / COPY_GBS / 1e3, 1)}
        if to:
            row.update({"other_path_us": round(statistics.median(to), 1), "other_path_launches": len(other), "direct_over_other": round(us / statistics.median(to), 3)})
        else:
            row["other_path"] = "cannot run: " + why
        return row
    finally:
        b.release()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sets", default="fcn,decoder"); ap.add_argument("--funcs", default="fwd,in,filts")
    ap.add_argument("--tile", default="", help="a seven-field tile 1xBJxBKx2x2x1xKSL for the direct call (use with --funcs filts): forced BK / KSL")
    ap.add_argument("--layers", default="", help="comma list: only the layers whose name contains one of these")
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
                    row = bench_layer(rtc, case, which, a.runs, a.warmup, a.blocks, tile=a.tile)
                    print(json.dumps(dict({"set": sn, "layer": layer, "case": list(case)}, **({"forced_tile": a.tile} if a.tile else {}), **row)), flush=True)
    finally:
        rtc.close()


if __name__ == "__main__":
    main()
