#!/usr/bin/env python3
"""Random-shape parity sweep of hip_conv_nhwc (channels-last bf16: implicit GEMM and the input-patch kernel, planner tiles and random forced tiles, float and
bf16 outputs) against the oracle on bf16-rounded operands, with the bounds of tests/test_gpu_nhwc.py.   usage: fuzz_nhwc.py [n_cases] [seed]   (GPU box)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from fuzz_fwd import nhwc_conv_draws   # the generator (tools/fuzz_fwd.py; tests/test_fwd_fuzz_cpu.py checks it)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    from boda_amd.cnn_op import OpTune
    from boda_amd.op import UnsupErr
    import test_gpu_nhwc as T
    from boda_amd.rtc import make_rtc
    from boda_amd.ops_prof import OpsBackend
    rtc = make_rtc("(be=hip)", 0); rtc.init(); be = OpsBackend(rtc)
    bad = 0; used = {}; done = 0
    draws = nhwc_conv_draws(seed)
    while done < n:
        sh, tile, f32 = next(draws); op = T._conv_op(*sh)
        try:
            outs, prc = T._run(be, op, OpTune(hip_tile=tile, **(T.NHWC_F32 if f32 else T.NHWC)))
        except UnsupErr as e:
            if tile: continue          # (a forced tile the layer's kernel does not take)
            bad += 1; done += 1; print("UNSUPPORTED", sh, str(e)[:200], flush=True); continue
        done += 1
        key = prc.launch["kernel"].replace("bodahip_", "") + " " + prc.launch["cfg"]; used[key] = used.get(key, 0) + 1
        try:
            (T._check_f32 if f32 else T._check_bf16)(op, outs, prc)
        except AssertionError as e:
            bad += 1; print("MISMATCH", sh, tile, "f32" if f32 else "bf16", str(e)[:300], flush=True)
    print(f"{n} cases, {bad} mismatches; kernels / tiles:", dict(sorted(used.items(), key=lambda kv: -kv[1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
