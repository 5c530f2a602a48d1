"""Times the non-conv functions of the gradient pipe on be=hip: the pooling and LRN layers of AlexNet and NiN at 256 images (forward-with-side-output and gradient:
hip_pool_yx / hip_spreading, hip_lrn_sb / hip_bck_lrn), the ReLU gradient on AlexNet's conv1 output, and the softmax loss at 256 x 1000.  Per function one JSON line: us
(median HIP-event time of --runs calls after --warmup), achieved GB/s from the algorithmic bytes (every tensor of the call read or written once), and that rate as a
fraction of the 6.29 TB/s copy rate measured on this chip (profiles/README.md).  No target is set: the record is the baseline later tuning is judged against.

    python tools/bck_ops_bench.py [--nets alexnet,nin] [--batch 256] [--runs 10] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boda_amd import conv_pipe  # noqa: E402
from boda_amd.cnn_op import NATIVE_ARGS, OpTune, add_bck_op_annotations  # noqa: E402
from boda_amd.op import Dims, Nda, Op  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402

COPY_TBS = 6.29   # measured device-to-device copy rate, profiles/README.md


def u32(v):
    return Nda(None, "uint32_t", (int(v),))


def f32(v):
    return Nda(None, "float", (float(v),))


def none(yx):
    return Nda(Dims(("y", "x"), tuple(yx), "none"), "none")


def layer_ops(cp, net):
    """(net, layer, op) for every max Pooling / LRN of the pipe as forward-with-side-output and gradient ops; average poolings as Spreading only."""
    out = []
    for o in cp.ops:
        i, t = cp.nodes[o.bot], cp.nodes[o.top]
        if o.type == "Pooling":
            base = {"in": Nda(i), "out": Nda(t), "kern_sz": none(o.kern_sz), "stride": none(o.stride), "in_pad": none(o.in_pad), "avg_pool": u32(o.avg_pool),
                    "emit_out_in_yx": u32(0 if o.avg_pool else 1)}
            if not o.avg_pool:
                out.append((net, o.tag, Op({"type": "Pooling"}, dict(base))))
            out.append((net, o.tag, Op({"type": "Spreading"}, dict(base, out_grad_loss=Nda(t), in_grad_loss=Nda(i)))))
        elif o.type == "LRN":
            ls, alpha, beta, k = o.lrn
            base = {"in": Nda(i), "out": Nda(i), "alpha": f32(alpha), "beta": f32(beta), "k": f32(k), "local_size": u32(ls), "emit_out_scale_base": u32(1)}
            out.append((net, o.tag, Op({"type": "LRN"}, dict(base))))
            out.append((net, o.tag, Op({"type": "BckLRN"}, dict(base, out_grad_loss=Nda(i), in_grad_loss=Nda(i)))))
    return out


def time_func(rtc, fop, rng, runs, warmup):
    """-> (median us, launch info).  Inputs: uniform values; out_in_yx / label hold valid indices; scale_base >= 1."""
    fn = fop.get_func_name()
    rtc.compile([RtcFuncInfo("f", "", [a for a, _ in NATIVE_ARGS[fn]], fop)])
    am, made = {}, []
    try:
        for an, io in NATIVE_ARGS[fn]:
            d = fop.get_dims(an)
            if io == "REF":
                am[an] = RtcArg.ref(d); continue
            rtc.create_var_with_dims(an, d); made.append(an); am[an] = RtcArg.var(an)
            if io == "IN":
                if an == "out_in_yx":
                    hw = fop.get_dims("in").dsz("y") * fop.get_dims("in").dsz("x")
                    v = rng.integers(0, hw, d.sizes).astype(np.float32)
                elif an == "label":
                    v = rng.integers(0, fop.get_dims("in").dsz("chan"), d.sizes).astype(np.float32)
                elif an == "out_scale_base":
                    v = rng.uniform(1.0, 2.0, d.sizes).astype(np.float32)
                elif an == "prob":
                    v = rng.uniform(0.0, 2.0 / d.dsz("chan"), d.sizes).astype(np.float32)
                else:
                    v = rng.uniform(-4, 4, d.sizes).astype(np.float32)
                rtc.copy_nda_to_var(an, v)
        call = RtcFuncCall("f", am)
        ids = [rtc.run(call) for _ in range(warmup + runs)]
        rtc.finish_and_sync()
        us = statistics.median(rtc.get_dur(c, c) * 1e3 for c in ids[warmup:])
        return us, rtc.last_launch()
    finally:
        for vn in made:
            rtc.release_var(vn)
        rtc.release_func("f"); rtc.release_per_call_id_data()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", default="alexnet,nin")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    ops = []
    for net in a.nets.split(","):
        make = {"alexnet": conv_pipe.alexnet_ng_conv, "nin": conv_pipe.nin_imagenet}.get(net)
        if make is None:
            raise SystemExit(f"unknown net {net!r}")
        ops += layer_ops(make(a.batch), net)
    relu = Dims.make("float", img=a.batch, chan=96, y=55, x=55)   # the ReLU gradient on AlexNet's conv1 output
    ops.append(("alexnet", "relu1", Op({"type": "ZeroIfNonPos"}, {"in": Nda(relu), "cond": Nda(relu), "out": Nda(relu)})))
    sm_in = Dims.make("float", img=a.batch, chan=1000, y=1, x=1)
    ops.append(("any", "loss", Op({"type": "SoftmaxWithLoss"}, {"in": Nda(sm_in), "in_grad_loss": Nda(sm_in), "label": Nda(Dims.make("float", img=a.batch, y=1, x=1)),
                                                               "loss": Nda(Dims.make("float", y=1, x=1))})))
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    rng = np.random.default_rng(0)
    for net, layer, op in ops:
        for f in add_bck_op_annotations(op, OpTune()):
            us, launch = time_func(rtc, f, rng, a.runs, a.warmup)
            gbs = launch["algo_bytes"] / (us * 1e-6) / 1e9
            i = f.get_dims("in")
            print(json.dumps({"net": net, "layer": layer, "func": f.get_func_name(), "in": "x".join(str(s) for s in i.sizes), "us": round(us, 2),
                              "algo_MB": round(launch["algo_bytes"] / 1e6, 2), "GBps": round(gbs, 1), "copy_frac": round(gbs / (COPY_TBS * 1e3), 3),
                              "kernel": launch["kernel"], "grid": launch["grid"]}), flush=True)
    rtc.close()


if __name__ == "__main__":
    main()
