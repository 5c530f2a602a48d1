"""The gradient step on several devices (img_shards=1) on the MI355X.  The devices are shards of device 0 (devices=0:0, 0:0:0, eight zeros), as
in the other multi-device tests; one test takes two distinct GPUs where there are two.

What a flagged call must leave is never taken from the multi-device backend: dropout, the loss gradient, loss_per_pel and loss are the ONE-device be=hip call's bits;
a filter / bias gradient is tests/bck_shards_ref.py's chain -- one-device be=hip calls of the unflagged function per image chunk, added in device order in numpy fp32 --
bit for bit, and within FILTS_MRD (tests/test_bck_conv_cpu.py) of float64.  Output vars hold NaN before every flagged call."""
import numpy as np
import pytest

import bck_pipe_ref as pref
import bck_shards_ref as sref
from boda_amd import rtc as rtc_mod
from boda_amd.bck_pipe import ConvPipeBck, add_bck_ops
from boda_amd.cnn_op import IMG_SHARDS_FUNCS, OpTune, add_bck_conv_annotations, add_bck_op_annotations, has_img_shards_flag, on_img_shards, seed_from_var
from boda_amd.conv_pipe import nin_imagenet
from boda_amd.op import UnsupErr
from boda_amd.rtc import make_rtc

from test_bck_conv_cpu import FILTS_MRD, bck_op, mrd, rand_ins, torch_grads
from test_bck_ops_cpu import labels, softmax_in, softmax_op
from test_bck_pipe_cpu import PIPES, SEED_A, SEED_B, dropout_op, small_inputs, small_params
from test_bck_shards_cpu import DROP_DIMS, GRAD_CASES, KSL_OP, LOSS_CASES, MULTI_OP, N_CLASS, ann, five

pytestmark = pytest.mark.gpu
bits_eq = sref.bits_eq


@pytest.fixture(scope="module")
def hip():
    r = make_rtc("(be=hip)", 0)
    r.init()
    yield r
    r.close()


@pytest.fixture(scope="module")
def multi():
    """n -> a backend over n shards of device 0, made on first use."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = make_rtc("(be=hip,devices=" + ":".join(["0"] * n) + ")"); made[n].init()
        return made[n]
    yield get
    for r in made.values():
        r.close()


def five_inputs():
    op = bck_op(3, 5, 9, 9, 7, 3, 3, 1, 1, 1, 1)
    g = rand_ins(op, 51)
    x = np.random.default_rng(52).uniform(-2, 2, (3, 5, 3, 5)).astype(np.float32)
    prob = softmax_in(3, N_CLASS, 0.0, 1.0, seed=53); prob /= prob.sum(axis=1, keepdims=True)
    return {"hip_bconv_filts": g, "hip_bconv_biases": g, "hip_dropout": {"inout": x}, "hip_sm_grad_and_loss": {"prob": prob, "label": labels(3, N_CLASS)},
            "hip_sum_loss_over_imgs": {"loss_per_pel": np.ones((3, 1, 1), np.float32)}}


# ---- flag absent: the refusals stay
def test_unflagged_functions_are_still_refused(multi):
    ins = five_inputs()
    msg = {"hip_bconv_filts": "cross-device reduction", "hip_bconv_biases": "cross-device reduction", "hip_sm_grad_and_loss": "GLOBAL image count",
           "hip_sum_loss_over_imgs": "over ALL images", "hip_dropout": "GLOBAL flat index"}
    for fn, f in five().items():
        assert not has_img_shards_flag(f)
        with pytest.raises(UnsupErr, match=msg[fn]):
            sref.run_func(multi(2), f, ins[fn], seed=1)


# ---- dropout
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("seed", [1, 0xffffffc0])     # the second: seed + a shard's first flat index (75, 150) wraps
@pytest.mark.parametrize("from_var", [False, True])
def test_dropout(hip, multi, n, seed, from_var):
    x = np.random.default_rng(61).uniform(-2, 2, (3, 5, 3, 5)).astype(np.float32)   # 75 elements per image: a shard's quads are not the whole tensor's
    fd = ann(dropout_op(0.5, DROP_DIMS))[0]
    if from_var:   # the word holds the seed, the call carries an offset by value: word + offset + the shard's base, all in wrapping uint32
        word, off = np.array([seed], np.uint32), 0x55
        want = sref.run_func(hip, seed_from_var(fd), {"inout": x, "det_drop_seed_var": word}, seed=off)["inout"]
        got = sref.run_func(multi(n), on_img_shards(seed_from_var(fd)), {"inout": x, "det_drop_seed_var": word}, seed=off)["inout"]
        assert bits_eq(want, pref.dropout_f32(x, 0.5, (seed + off) & 0xFFFFFFFF))
    else:
        want = sref.run_func(hip, fd, {"inout": x}, seed=seed)["inout"]
        got = sref.run_func(multi(n), on_img_shards(fd), {"inout": x}, seed=seed)["inout"]
        assert bits_eq(want, pref.dropout_f32(x, 0.5, seed))
    assert bits_eq(got, want) and np.any(got == 0) and np.any(got != 0)


# ---- the loss gradient and the loss
@pytest.mark.parametrize("T,n", LOSS_CASES)
def test_loss_gradient_and_loss(hip, multi, T, n):
    fs, fg, fl = add_bck_op_annotations(softmax_op(T, N_CLASS), OpTune())
    prob = sref.run_func(hip, fs, {"in": softmax_in(T, N_CLASS, seed=62)})["prob"]
    lab = labels(T, N_CLASS, seed=T); lab[T - 1] = N_CLASS + 3            # a label outside [0, chan): no channel matches, loss_per_pel = -logf(FLT_MIN)
    one = sref.run_func(hip, fg, {"prob": prob, "label": lab})
    two = sref.run_func(multi(n), on_img_shards(fg), {"prob": prob, "label": lab})
    assert bits_eq(two["in_grad_loss"], one["in_grad_loss"]) and bits_eq(two["loss_per_pel"], one["loss_per_pel"])
    assert bits_eq(one["in_grad_loss"].reshape(T, -1)[0, 1:2], (prob.reshape(T, -1)[0, 1:2] / np.float32(T)).astype(np.float32))   # the divisor is T, whatever the shard holds
    lpp = one["loss_per_pel"].copy(); lpp[0] = 2.0 ** 24                 # 2^24 + 1 + ... : the one chain from +0 in image order, not a sum of per-shard sums
    want = sref.run_func(hip, fl, {"loss_per_pel": lpp})["loss"]
    got, copies = sref.run_func(multi(n), on_img_shards(fl), {"loss_per_pel": lpp}, then=lambda r, am: sref.probe_copies(r, am["loss"].n, n))
    assert bits_eq(got["loss"], want)
    for i in range(n):
        assert bits_eq(copies[i], want.reshape(-1)), i                   # every device's copy of `loss`


# ---- the filter and bias gradients
@pytest.mark.parametrize("shape,n", [(s, n) for s, ns in GRAD_CASES for n in ns])
def test_filter_and_bias_gradients(hip, multi, shape, n):
    op = bck_op(*shape)
    ins = rand_ins(op, sum(shape) + n)
    _, fb, ff = add_bck_conv_annotations(op, OpTune())
    if shape == KSL_OP:   # the per-shard plans must cut K: read from the planner, so that the case cannot silently lose its slices
        ksl = [int(rtc_mod.explain_plan(sref.chunk_op(ff, e - b)).split("ksl=")[1].split()[0]) for b, e in sref.chunks(shape[0], n)]
        assert min(ksl) > 1 and len(set(ksl)) > 1, ksl
    _, gw, gb = torch_grads(op, ins["in"], ins["filts"], ins["out_grad_loss"])
    for f, f64 in ((ff, gw), (fb, gb)):
        an = sref.grad_arg(f)
        fins = {"in": ins["in"], "out_grad_loss": ins["out_grad_loss"]}   # (the bias gradient reads only the second)
        want = sref.sharded_grad(hip, f, fins, n)
        got, copies = sref.run_func(multi(n), on_img_shards(f), fins, then=lambda r, am: sref.probe_copies(r, am[an].n, n))
        print(f"{shape} over {n} {an}: mrd {mrd(got[an], f64):.3e}")
        assert bits_eq(got[an], want), an
        assert mrd(got[an], f64) < FILTS_MRD, an
        for i in range(n):   # every device's copy, shards without images included
            assert bits_eq(copies[i], (want + np.float32(0)).reshape(-1)), (an, i)


# ---- the whole step
def step_nodes(bp):
    return [n for n, d in bp.nodes.items() if d.names and d.names[0] == "img"] + list(bp.loss_nodes) + [n for n in bp.nodes if n.endswith(("_filts_grad_loss", "_biases_grad_loss"))]


def check_step(hip, rtc_m, n, cp, tops, params, rounds, **kw):
    """One driver on one device, one on n shards; per round (drop seed, data, label): every img-leading node and every loss bit-identical, every filter / bias gradient
    the helper's chain over the one-device step's own in / out_grad_loss nodes."""
    bp1, bpm = add_bck_ops(cp, loss_tops=tops), add_bck_ops(cp, loss_tops=tops)
    d1 = ConvPipeBck(hip, **kw); dm = ConvPipeBck(rtc_m, **kw)
    try:
        d1.init(bp1, params); dm.init(bpm, params)
        assert not any(has_img_shards_flag(f) for _, f, _ in d1.calls())
        assert all(has_img_shards_flag(f) == (f.get_func_name() in IMG_SHARDS_FUNCS) for _, f, _ in dm.calls())
        gets = step_nodes(bp1)
        for seed, data, label in rounds:
            outs = []
            for d in (d1, dm):
                for v in gets:   # NaN everywhere a call must write
                    d.rtc.copy_nda_to_var(v, np.full(bp1.nodes[v].sizes, np.nan, np.float32))
                d.set_det_drop_seed(seed)
                fwd = {"data": data, "label": label}
                d.run_bck(["data", "label"], fwd, gets)
                outs.append(fwd)
            one, many = outs
            grads = {}
            for c in d1.bck_calls:
                if c.fop.get_func_name() in ("hip_bconv_filts", "hip_bconv_biases"):
                    an = sref.grad_arg(c.fop)
                    fins = {a: hip.copy_var_to_nda(c.args[a]) for a in c.args if a != an}
                    grads[c.args[an]] = sref.sharded_grad(hip, c.fop, fins, n)
            assert len(grads) == len(cp.params)
            for v in gets:
                assert np.all(np.isfinite(many[v])), v
                assert bits_eq(many[v], grads[v] if v in grads else one[v]), (seed, v)
        return one, many
    finally:
        d1.release(); dm.release()


def small_rounds(cp):
    return [(seed, *small_inputs(cp, 20 + r)) for r, seed in enumerate((SEED_A, SEED_B))]


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("name", sorted(PIPES))
def test_small_pipes_on_three_shards(hip, multi, name, B, fuse):
    mk, tops, pseed = PIPES[name]
    cp = mk(B)
    one, many = check_step(hip, multi(3), 3, cp, tops, small_params(cp, pseed), small_rounds(cp), fuse_relu_grad=fuse)
    assert np.any(many["data_grad_loss"] != 0)


def test_small_pipe_seed_in_var(hip, multi):
    cp = PIPES["chain"][0](3)
    check_step(hip, multi(3), 3, cp, None, small_params(cp, 0), small_rounds(cp), seed_in_var=True)


def test_nin_two_images_on_two_shards(hip, multi):
    cp = nin_imagenet(2)
    from boda_amd.bck_pipe import host_params
    rng = np.random.default_rng(0)
    data = rng.uniform(-1, 1, cp.nodes["data"].sizes).astype(np.float32)
    label = np.array([3, 998], np.float32).reshape(2, 1, 1)
    one, many = check_step(hip, multi(2), 2, cp, None, host_params(add_bck_ops(cp), 5), [(5, data, label)])
    assert np.any(many["conv1_filts_grad_loss"] != 0) and np.isfinite(many["loss"]).all()


# ---- other
def test_capture_graph_is_refused(multi):
    cp = PIPES["fan"][0](3)
    drv = ConvPipeBck(multi(3)); drv.init(add_bck_ops(cp), small_params(cp, 0))
    try:
        with pytest.raises(UnsupErr, match="multi-device"):
            drv.capture_graph()
    finally:
        drv.release()


def test_forced_peer_copies(hip, monkeypatch):
    """BODAHIP_FORCE_PEER=1: the copies between shards of one GPU take hipMemcpyPeerAsync, the path of distinct GPUs.  Same bits."""
    monkeypatch.setenv("BODAHIP_FORCE_PEER", "1")
    r = make_rtc("(be=hip,devices=0:0:0)"); r.init()
    try:
        cp = PIPES["chain"][0](3)
        check_step(hip, r, 3, cp, None, small_params(cp, 0), small_rounds(cp)[:1])
    finally:
        r.close()


def test_two_distinct_gpus(hip):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the one-GPU box covers the same code path with shards of device 0 and BODAHIP_FORCE_PEER)")
    r = make_rtc("(be=hip,devices=0:1)"); r.init()
    try:
        cp = PIPES["heads"][0](3)
        check_step(hip, r, 2, cp, PIPES["heads"][1], small_params(cp, 0), small_rounds(cp)[:1])
    finally:
        r.close()
