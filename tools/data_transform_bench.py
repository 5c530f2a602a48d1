"""Times hip_data_transform on be=hip at the inputs a training run feeds: AlexNet's (256 images 256 x 256 x 3 -> 227) and ResNet-50's (32 and 64 images 256 x 256 x 3 ->
224), under both source layouts and both mean forms, beside hip_chan_affine on the same float tensor (in -> out, the plainest streaming function of the pipe) and the
uploads the transform replaces.  One process; the functions of one input are timed in alternating blocks (--blocks rounds of --runs calls each, every function once per
round), so that a drift of the machine falls on all of them alike.  Per function one JSON line: us (the median HIP-event time over all blocks), GB/s from the algorithmic
bytes (hip_data_transform: one source byte read and one float written per output element, the plan, and the mean -- one float per output element where it is per pel,
the C values once where it is per channel; hip_chan_affine: every tensor once), and that rate as a fraction of the 6.29 TB/s copy rate of profiles/README.md, as
tools/bck_ops_bench.py reports it.  Per input one more line: the median host time (a clock around copy_nda_to_var + finish_and_sync) of uploading the uint8 batch and
of uploading the float batch it replaces.  No gate hangs on any of this.

    python tools/data_transform_bench.py [--inputs alexnet256,resnet32,resnet64] [--blocks 5] [--runs 10] [--warmup 3] [--uploads 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from boda_amd.cnn_op import chan_affine_func_op, data_transform_func_op, pipe_func_args  # noqa: E402
from boda_amd.op import Dims  # noqa: E402
from boda_amd.rtc import RtcArg, RtcFuncCall, RtcFuncInfo, make_rtc  # noqa: E402

COPY_TBS = 6.29   # measured device-to-device copy rate, profiles/README.md
INPUTS = {"alexnet256": (256, 227), "resnet32": (32, 224), "resnet64": (64, 224)}   # name -> (images, crop); the source is 256 x 256 x 3


class Func:
    """One compiled function with vars of its own, filled once."""

    def __init__(self, rtc, name, fop, fill):
        self.rtc, self.name, self.fop, self.vars = rtc, name, fop, []
        spec = [(an, io) for an, io in pipe_func_args(fop)]
        rtc.compile([RtcFuncInfo(name, "", [a for a, _ in spec], fop)])
        am = {}
        for an, io in spec:
            vn = f"{name}_{an}"
            rtc.create_var_with_dims(vn, fop.get_dims(an)); self.vars.append(vn); am[an] = RtcArg.var(vn)
            if io == "IN":
                rtc.copy_nda_to_var(vn, fill(an, fop.get_dims(an)))
        self.call = RtcFuncCall(name, am)
        self.us = []
        self.launch = None

    def block(self, runs, keep=True):
        ids = [self.rtc.run(self.call) for _ in range(runs)]
        self.rtc.finish_and_sync()
        if keep:
            self.us += [self.rtc.get_dur(c, c) * 1e3 for c in ids]
        self.launch = self.rtc.last_launch()
        self.rtc.release_per_call_id_data()

    def release(self):
        for vn in self.vars:
            self.rtc.release_var(vn)
        self.rtc.release_func(self.name)


def upload_ms(rtc, vn, a, n):
    ts = []
    for _ in range(n):
        rtc.finish_and_sync()
        t0 = time.perf_counter()
        rtc.copy_nda_to_var(vn, a); rtc.finish_and_sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", default="alexnet256,resnet32,resnet64")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--uploads", type=int, default=5)
    a = ap.parse_args(argv)
    rtc = make_rtc("(be=hip)", 0)
    rtc.init()
    rng = np.random.default_rng(0)
    H = W = 256; C = 3

    def fill(an, d):
        if d.tn == "uint8_t":
            return rng.integers(0, 256, d.sizes, dtype=np.uint8)
        if an == "plan":     # a train plan's shape: offsets all over the range, every other image mirrored
            p = np.zeros(d.sizes, np.uint32)
            p[:, 0] = rng.integers(0, 30, d.sizes[0]); p[:, 1] = rng.integers(0, 30, d.sizes[0]); p[:, 2] = np.arange(d.sizes[0]) & 1
            return p
        return rng.uniform(90, 130, d.sizes).astype(np.float32)

    for name in a.inputs.split(","):
        if name not in INPUTS:
            raise SystemExit(f"unknown input {name!r}")
        B, crop = INPUTS[name]
        funcs = []
        for layout in ("hwc", "chw"):
            sd = Dims.make("uint8_t", img=B, y=H, x=W, chan=C) if layout == "hwc" else Dims.make("uint8_t", img=B, chan=C, y=H, x=W)
            for form, md in (("chan", Dims.make("float", chan=C)), ("chan:y:x", Dims.make("float", chan=C, y=H, x=W))):
                funcs.append((f"{layout} mean={form}", Func(rtc, f"xf{len(funcs)}", data_transform_func_op(sd, (crop, crop), md, 0.017), fill)))
        od = Dims.make("float", img=B, chan=C, y=crop, x=crop)
        funcs.append(("", Func(rtc, "aff", chan_affine_func_op(od, 0), fill)))
        for _, f in funcs:
            f.block(a.warmup, keep=False)
        for _ in range(a.blocks):     # alternating blocks: every function once per round
            for _, f in funcs:
                f.block(a.runs)
        for form, f in funcs:
            us = statistics.median(f.us)
            gbs = f.launch["algo_bytes"] / (us * 1e-6) / 1e9
            print(json.dumps({"input": name, "func": f.fop.get_func_name(), "form": form, "out": "x".join(str(s) for s in od.sizes), "us": round(us, 2),
                              "us_min": round(min(f.us), 2), "us_max": round(max(f.us), 2), "algo_MB": round(f.launch["algo_bytes"] / 1e6, 2), "GBps": round(gbs, 1),
                              "copy_frac": round(gbs / (COPY_TBS * 1e3), 3), "kernel": f.launch["kernel"], "grid": f.launch["grid"]}), flush=True)
        raw = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
        flt = rng.uniform(-1, 1, od.sizes).astype(np.float32)
        u8_ms = upload_ms(rtc, "xf0_src", raw, a.uploads)
        f32_ms = upload_ms(rtc, "aff_in", flt, a.uploads)
        print(json.dumps({"input": name, "upload_uint8_MB": round(raw.nbytes / 1e6, 1), "upload_uint8_ms": round(u8_ms, 2), "upload_float_MB": round(flt.nbytes / 1e6, 1),
                          "upload_float_ms": round(f32_ms, 2)}), flush=True)
        for _, f in funcs:
            f.release()
    rtc.close()


if __name__ == "__main__":
    main()
