#!/usr/bin/env python3
"""Interleaved A/B of sgemm plans, one process, one device: for every size the operands are made once, then the arms take turns -- ROUNDS visits each, every visit ITERS
back-to-back launches, the visit's figure their median.  Per arm: the median over the visits and their spread (min .. max).  An arm is a set of environment variables the
planner reads at every call (BODAHIP_SGEMM_TILE_FOR, BODAHIP_SGEMM_PARTS, BODAHIP_NO_SGEMM_W12, BODAHIP_EXTRA_DEFS ...).
usage: python tools/sgemm_plan_ab.py --sizes 6144,12288 --arm "parent:BODAHIP_NO_SGEMM_W12=1 BODAHIP_EXTRA_DEFS=-DSTGRING=0" --arm new: [--rounds 5] [--iters 4] [--settle-ms 300]"""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from boda_amd import gen_data as gd
from boda_amd.cnn_op import OpTune, add_codegen_annotations
from boda_amd.op import parse_op
from boda_amd.ops_prof import OpsBackend
from boda_amd.rtc import RtcArg, RtcFuncCall, make_rtc

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="6144,12288,8192,10240,7168")
ap.add_argument("--arm", action="append", default=[], help="'name:VAR=value VAR=value' ({n} in a value stands for the size)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=4)
ap.add_argument("--settle-ms", type=float, default=300.0)
a = ap.parse_args()
arms = []
for spec in a.arm:
    name, _, rest = spec.partition(":")
    arms.append((name, dict(kv.split("=", 1) for kv in rest.split())))
rtc = make_rtc(); rtc.init(); be = OpsBackend(rtc)


def run_arm(rfc, env, n, iters):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: v.replace("{n}", str(n)) for k, v in env.items()})
    try:
        ids = [rtc.run(rfc) for _ in range(iters)]
        launch = rtc.last_launch()
        rtc.finish_and_sync()
        return [rtc.get_dur(i, i) / 1000.0 for i in ids], launch
    finally:
        for k, v in old.items():
            if v is None: del os.environ[k]
            else: os.environ[k] = v


for n in (int(x) for x in a.sizes.split(",")):
    op = add_codegen_annotations(parse_op(f"(str_vals=(type=sgemm),nda_vals=(a=(dims=(K={n},M={n})),b=(dims=(K={n},N={n})),c=(dims=(M={n},N={n}))))"), OpTune())
    fn = be.gen_func(op)
    for an in "abc": rtc.create_var_with_dims(an, op.get_dims(an))
    for an in "ab": rtc.run(gd.gen_call("sgemm", an, an, op.get_dims(an), 5, 0.0))
    rfc = RtcFuncCall(fn, {an: RtcArg.var(an) for an in "abc"})
    cfgs = {}
    for name, env in arms:   # (first use: code objects load / compile here, untimed)
        _, launch = run_arm(rfc, env, n, 1); cfgs[name] = f"{launch['cfg']} grid {launch['grid']}"
    t0 = time.time()
    while (time.time() - t0) * 1e3 < a.settle_ms: run_arm(rfc, arms[0][1], n, 2)   # sustained load before the timed visits: clocks settle
    vis = {name: [] for name, _ in arms}
    for r in range(a.rounds):
        for name, env in arms:
            secs, _ = run_arm(rfc, env, n, a.iters); vis[name].append(statistics.median(secs))
    fl = 2.0 * n * n * n
    for name, _ in arms:
        v = vis[name]; med = statistics.median(v)
        print(f"{n:6d}^3 {name:8s} [{cfgs[name]:>40s}] median {med * 1e3:8.4f} ms = {fl / med / 1e12:6.2f} TF/s   visits {min(v) * 1e3:8.4f} .. {max(v) * 1e3:8.4f} ms "
              f"(spread {(max(v) - min(v)) / med * 100:4.2f} %)   " + " ".join(f"{x * 1e3:.4f}" for x in v), flush=True)
    rtc.finish_and_sync()
    for an in "abc": rtc.release_var(an)
    rtc.release_per_call_id_data(); be.gc_clear()
