"""boda_amd/cnn_op.py's tables of the native functions held to the backend's one table (csrc/native_funcs.h), read through bodahip_native_funcs / bodahip_func_args:
names, op flags, call order, arg lists, optional args and the multi-device refusal sentences.  cnn_op.py imports no library, so its tables stay; nothing is generated."""
import os
import re

import pytest

import fwd_deps_ref
from boda_amd import rtc as rtc_mod
from boda_amd.cnn_op import (BCK_OP_FUNCS, BCONV_FB_FUNC, BCONV_FUNCS, BN_OP_FUNCS, IMG_SHARDS_FUNCS, NATIVE_ARGS, PIPE_OP_FUNCS, SGD_OP_FUNCS, ZINP_FUNCS, OpTune,
                             add_bck_conv_annotations, add_bck_op_annotations, bn_bck_in_func_op, bn_bck_sums_func_op, bn_fwd_func_op, bn_stats_func_op, chan_affine_func_op,
                             fan_out_func_op, fuse_zero_if_in_non_pos, on_img_shards, pipe_func_args, seed_from_var, sgd_update_func_op)
from boda_amd.op import Dims, Nda, Op, read_ops
from boda_amd.rtc import RtcFuncInfo, make_rtc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ops")
MEMBER_LIST_FUNCS = {"hip_conv_nhwc_grp", "hip_conv_nhwc_multi", "hip_conv_nhwc_set"}   # their arg lists are lists of members: described by their handlers (boda_amd/nhwc.py)


@pytest.fixture(scope="module")
def table():
    return rtc_mod.native_funcs()   # (a name with two rows is an RtErr there)


def ops_of(fn):
    return read_ops(os.path.join(GOLD, fn))


def with_flag(table, flag):
    return {n for n, r in table.items() if flag in r["flags"]}


def test_names(table):
    assert set(NATIVE_ARGS) <= set(table)
    cpu_own = {n for n in table if n.startswith("cpu_")}
    assert cpu_own == {"cpu_sgemm", "cpu_conv_fwd"} and all(table[n]["be"] == ("cpu",) for n in cpu_own)
    assert set(table) - MEMBER_LIST_FUNCS - cpu_own == set(NATIVE_ARGS)
    assert MEMBER_LIST_FUNCS <= set(table)


def test_flags(table):
    assert with_flag(table, "zero_if_in_non_pos") == set(ZINP_FUNCS)
    assert with_flag(table, "img_shards") == set(IMG_SHARDS_FUNCS)
    assert with_flag(table, "seed_from_var") == {"hip_dropout"}
    assert with_flag(table, "nhwc_residual") == {"hip_conv_nhwc"}
    assert {f for r in table.values() for f in r["flags"]} == {"zero_if_in_non_pos", "img_shards", "seed_from_var", "nhwc_residual"}


def test_call_order(table):
    """A bare op's calls are its type's rows in ascending member (native_funcs.h): the reference's call order."""
    by_type = {}
    for name, r in sorted(table.items(), key=lambda kv: kv[1]["member"]):   # (stable: table order within a member)
        if "hip" in r["be"]:
            for t in r["types"]:
                by_type.setdefault((r["family"], t), []).append(name)
    got = lambda fam: {t: tuple(v) for (f, t), v in by_type.items() if f == fam}
    assert got("bck_op") == {**BCK_OP_FUNCS, **PIPE_OP_FUNCS, "ChanAffine": ("hip_chan_affine",)}
    assert got("bn") == BN_OP_FUNCS
    assert got("sgd") == SGD_OP_FUNCS
    assert got("bconv") == {"BckConv": BCONV_FUNCS + (BCONV_FB_FUNC,)}   # (the fused gradient, opt-in, is behind the three calls of the bare op)
    assert [table[n]["member"] for n in BCONV_FUNCS] == [1, 2, 3]


def func_ops():
    """Every function op the issue names: the annotators' on the golden op lists, the func_op constructors at one small shape, and every legal flagged form."""
    tune = OpTune()
    fops = []
    for op in ops_of("bck-conv-ops.txt"):
        fops += add_bck_conv_annotations(op, tune)
    fops += ops_of("bconv-fb-ops.txt")
    for op in ops_of("bck-ops.txt"):
        fops += add_bck_op_annotations(op, tune)
    for fn in ("bck-pipe-ops.txt", "bck-fuse-ops.txt", "bck-graph-ops.txt", "bck-shards-ops.txt", "bn-ops.txt", "sgd-ops.txt", "resnet-ops.txt"):   # (annotated function ops, flagged ones among them)
        fops += ops_of(fn)
    d = Dims(("img", "chan", "y", "x"), (2, 4, 3, 5), "float")
    fops += [chan_affine_func_op(d, 1), sgd_update_func_op([d]), sgd_update_func_op([d] * 32), bn_stats_func_op(d, 1e-5, 0.9), bn_fwd_func_op(d, 1), bn_bck_sums_func_op(d),
             bn_bck_in_func_op(d), fan_out_func_op(d, 2), fan_out_func_op(d, 8)]
    flagged = []
    for f in fops:
        fn = f.get_func_name()
        if fn in ZINP_FUNCS and not f.has("zero_if_in_non_pos") and f.get_dims("in") == f.get_dims("in_grad_loss"):
            flagged.append(fuse_zero_if_in_non_pos(f))
        if fn == "hip_dropout" and not f.has("seed_from_var"):
            flagged += [seed_from_var(f), on_img_shards(seed_from_var(f))]
        if fn in IMG_SHARDS_FUNCS and not f.has("img_shards"):
            flagged.append(on_img_shards(f))
        if fn == "hip_conv_nhwc" and not f.has("nhwc_residual") and len(f.get_dims("filts").names) == 4:
            r = f.copy(); r.nda_vals["nhwc_residual"] = Nda(None, "uint32_t", (1,)); r.nda_vals["res"] = r.get("out"); flagged.append(r)
    return fops + flagged


def test_arg_lists(table):
    fops = func_ops()
    seen = set()
    flag_forms = set()
    for f in fops:
        key = f.to_str()
        if key in seen:
            continue
        seen.add(key)
        assert rtc_mod.func_args(f) == pipe_func_args(f), key
        flag_forms |= {(f.get_func_name(), fl) for fl in ("zero_if_in_non_pos", "seed_from_var", "img_shards", "nhwc_residual") if f.has(fl) and f.get_u32(fl)}
    assert {f.get_func_name() for f in fops} <= set(NATIVE_ARGS)
    assert flag_forms == {(n, fl) for n, r in table.items() for fl in r["flags"]}   # every legal flagged form was compared
    missing = set(NATIVE_ARGS) - {f.get_func_name() for f in fops}   # functions no golden list holds: their fixed lists, on an op that carries nothing else
    for fn in sorted(missing):
        assert rtc_mod.func_args(Op({"type": table[fn]["types"][0], "func_name": fn}, {})) == NATIVE_ARGS[fn], fn


def test_optional_args(table):
    assert {n: {r["opt"][0]: r["opt"][1]} for n, r in table.items() if r["opt"]} == fwd_deps_ref.OPTIONAL_NATIVE


def gpu_test_matches(fn, pattern):
    src = open(os.path.join(HERE, fn)).read()
    return re.findall(pattern, src)


def test_refusal_sentences(table):
    """The sentence a multi-device backend answers with is the row's; be=cpu (one shard) accepts the unflagged function.  The GPU tests' match= strings, read from their
    files, must find their sentence in the table."""
    want = set(IMG_SHARDS_FUNCS)
    assert {n for n, r in table.items() if r["multi_dev"] == "needs_flag"} == want
    refused = {n for n, r in table.items() if r["multi_dev"] == "refused"}
    assert refused == {BCONV_FB_FUNC} | {v[0] for v in BN_OP_FUNCS.values()}
    assert {n for n, r in table.items() if r["multi_dev"] == "replicated_only"} == {"hip_sgd_update"}
    for n, r in table.items():
        assert bool(r["why"]) == (r["multi_dev"] in ("needs_flag", "refused")), n
    # tests/test_gpu_bck_shards.py: msg = {"<function>": "<match>", ...}
    pairs = gpu_test_matches("test_gpu_bck_shards.py", r'"(hip_\w+)": "([^"]+)"')
    msg = {fn: m for fn, m in pairs if fn in want}
    assert set(msg) == want
    for fn, m in msg.items():
        assert re.search(m, table[fn]["why"]), (fn, m)
    # tests/test_gpu_bn.py: (<constructor>(...), {...}, "<match>") per function
    bn = gpu_test_matches("test_gpu_bn.py", r'\((bn_\w+|fan_out)_func_op\(.*?, "([^"]+)"\)')
    ctor = {"bn_stats": "hip_bn_stats", "bn_bck_sums": "hip_bn_bck_sums", "bn_bck_in": "hip_bn_bck_in", "bn_fwd": "hip_bn_fwd", "fan_out": "hip_fan_out"}
    assert {ctor[c] for c, _ in bn} == refused - {BCONV_FB_FUNC}
    for c, m in bn:
        assert re.search(m, table[ctor[c]]["why"]), (c, m)
    # tests/test_gpu_bconv_fb.py: test_two_shards_refuse_it_by_name
    (m,) = gpu_test_matches("test_gpu_bconv_fb.py", r'(?s)def test_two_shards_refuse_it_by_name\(\):.*?match="([^"]+)"')
    assert re.search(m, table[BCONV_FB_FUNC]["why"])
    # be=cpu compiles every one of them unflagged
    by_fn = {}
    for f in func_ops():
        if not any(f.has(fl) and f.get_u32(fl) for fl in ("img_shards", "seed_from_var", "zero_if_in_non_pos")):
            by_fn.setdefault(f.get_func_name(), f)
    cpu = make_rtc("(be=cpu)"); cpu.init()
    try:
        for i, fn in enumerate(sorted(want | refused)):
            f = by_fn[fn]
            cpu.compile([RtcFuncInfo(f"nf_{i}", "", [a for a, _ in pipe_func_args(f)], f)])
    finally:
        cpu.close()
