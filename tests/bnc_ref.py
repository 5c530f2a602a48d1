"""What the tests of the training BatchNorm over img chunks share (tests/test_bnc_cpu.py, tests/test_gpu_bnc.py): the numpy twin of the CHUNKED chain of the three
per-channel sums (boda_amd/csrc/kernels/bn_f32.hip), built from bn_ref's chain_sum and slab_plan per chunk, the case matrix, and a runner of
the four hip_bnc_* functions on one backend.  Everything that is not the order of the sums -- the formulas, the element-wise functions, the float64 bounds -- is
bn_ref's, which this file imports and does not edit.

The chain: the batch of T images is cut into n chunks, chunk i = images [T * i // n, T * (i + 1) // n).  Inside a chunk a channel's elements are numbered from the
chunk's first image and the slab plan is the plan of the chunk's own dims; bn_ref.chain_sum gives the chunk total D_i; the channel's sum is ((D_a + D_b) + D_c) + ...
over the non-empty chunks in ascending order starting from the first.  fN, the unbiasing factor, the N == 1 case and the mean of S2's terms are the whole batch's."""
import numpy as np

import bn_ref
from bn_ref import EPS, F, MAF, bc, chain_sum, chan_terms, dims_of, make_inputs, run_func, same_bits, slab_plan
from boda_amd.cnn_op import bnc_bck_in_func_op, bnc_bck_sums_func_op, bnc_fwd_func_op, bnc_stats_func_op

# (shape, chunks, forced slab): N = 1 and an empty chunk | chunk 0 empty | odd planes, chunks of 1 and 2 images | a forced slab | several slabs per chunk | two ragged
# slabs per chunk, the planner's plan one | chunks >> images
CASES = [((1, 1, 1, 1), 2, 0), ((2, 4, 2, 2), 3, 0), ((3, 5, 3, 3), 2, 0), ((3, 5, 3, 3), 3, 0), ((3, 2, 7, 7), 3, 48), ((5, 65, 4, 4), 2, 16), ((5, 65, 4, 4), 3, 16),
         ((2, 3, 57, 57), 2, 2000), ((5, 3, 3, 3), 64, 0)]
case_id = lambda c: "x".join(map(str, c[0])) + f"_chunks{c[1]}_slab{c[2]}"


def chunks(T, n):
    """-> [(first image, end image)] of the n chunks of a batch of T images, empty ones included."""
    return [(T * i // n, T * (i + 1) // n) for i in range(n)]


def chunked_sum(t, c, n, forced=0):
    """The chunked chain over channel c of the term tensor t (img, chan, y, x) -> np.float32."""
    B, C, H, W = t.shape
    tot = None
    for b0, b1 in chunks(B, n):
        if b1 == b0:
            continue
        slab, _ = slab_plan(C, (b1 - b0) * H * W, forced)
        d = chain_sum(chan_terms(t[b0:b1], c), slab)
        tot = d if tot is None else F(tot + d)
    assert tot.dtype == F
    return tot


def stats_np(x, run_mean, run_var, n, eps=EPS, maf=MAF, forced=0):
    """-> mean, inv_std, run_mean', run_var': bn_ref.stats_np with S1 and S2 in the chunked chain."""
    B, C, H, W = x.shape
    N = B * H * W
    fN, omm = F(N), F(1) - F(maf)
    unb = fN / F(N - 1) if N > 1 else F(1)
    mean = np.zeros(C, F); istd = np.zeros(C, F); rm = np.zeros(C, F); rv = np.zeros(C, F)
    for c in range(C):
        m = chunked_sum(x, c, n, forced) / fN
        d = x - m
        var = chunked_sum(d * d, c, n, forced) / fN
        ve = var + F(eps)
        sd = np.sqrt(ve)
        mean[c] = m; istd[c] = F(1) / sd
        rm[c] = F(maf) * run_mean[c] + omm * m
        uv = var if N == 1 else var * unb
        rv[c] = F(maf) * run_var[c] + omm * uv
        assert all(v.dtype == F for v in (m, var, ve, sd, uv))
    return mean, istd, rm, rv


def bck_sums_np(x, mean, istd, dy, n, forced=0):
    C = x.shape[1]
    xh = (x - bc(mean)) * bc(istd)
    t = dy * xh
    sg = np.array([chunked_sum(t, c, n, forced) for c in range(C)], F)
    bg = np.array([chunked_sum(dy, c, n, forced) for c in range(C)], F)
    return sg, bg


def run_all_four(rtc, shape, n, forced=0, relu=1, seed=0, repeat=1, inputs=None):
    """bn_ref.run_all_five for the four hip_bnc_* functions with chunks=n, each fed the BACKEND's own upstream results -> dict of everything."""
    d = dims_of(shape)
    i = inputs if inputs is not None else make_inputs(shape, seed)
    r = dict(i)
    sts = run_func(rtc, bnc_stats_func_op(d, EPS, MAF, n, forced), {"in": i["x"], "run_mean": i["run_mean"], "run_var": i["run_var"]}, repeat=repeat)
    for s in sts[1:]:     # (the running pair moves on; the batch statistics must not)
        assert same_bits(s["mean"], sts[0]["mean"]) and same_bits(s["inv_std"], sts[0]["inv_std"]), "a repeated launch on the same workspace changed bits"
    st = sts[0]
    r.update(mean=st["mean"], inv_std=st["inv_std"], run_mean2=st["run_mean"], run_var2=st["run_var"])
    if repeat > 1:
        r.update(run_mean3=sts[1]["run_mean"], run_var3=sts[1]["run_var"])
    common = {"in": i["x"], "mean": r["mean"], "inv_std": r["inv_std"]}
    r["out"] = run_func(rtc, bnc_fwd_func_op(d, relu), dict(common, scale=i["scale"], bias=i["bias"]))[0]["out"]
    sums = run_func(rtc, bnc_bck_sums_func_op(d, n, forced), dict(common, out_grad_loss=i["dy"]), repeat=repeat)
    for s in sums[1:]:
        assert same_bits(s["scale_grad_loss"], sums[0]["scale_grad_loss"]) and same_bits(s["bias_grad_loss"], sums[0]["bias_grad_loss"]), "a repeated launch on the same workspace changed bits"
    r.update(sg=sums[0]["scale_grad_loss"], bg=sums[0]["bias_grad_loss"])
    r["dx"] = run_func(rtc, bnc_bck_in_func_op(d), dict(common, scale=i["scale"], scale_grad_loss=r["sg"], bias_grad_loss=r["bg"], out_grad_loss=i["dy"]))[0]["in_grad_loss"]
    return r


def check_against_numpy(r, shape, n, forced=0, relu=1):
    """Every result of run_all_four against the twin, each stage fed the twin's own upstream results (equal bits upstream make them the backend's too)."""
    mean, istd, rm, rv = stats_np(r["x"], r["run_mean"], r["run_var"], n, EPS, MAF, forced)
    assert same_bits(r["mean"], mean), "mean"
    assert same_bits(r["inv_std"], istd), "inv_std"
    assert same_bits(r["run_mean2"], rm) and same_bits(r["run_var2"], rv), "running pair"
    if "run_mean3" in r:     # (the second call moves the running pair on from the first call's)
        _, _, rm3, rv3 = stats_np(r["x"], rm, rv, n, EPS, MAF, forced)
        assert same_bits(r["run_mean3"], rm3) and same_bits(r["run_var3"], rv3), "running pair after two calls"
    assert same_bits(r["out"], bn_ref.fwd_np(r["x"], mean, istd, r["scale"], r["bias"], relu)), "out"
    sg, bg = bck_sums_np(r["x"], mean, istd, r["dy"], n, forced)
    assert same_bits(r["sg"], sg) and same_bits(r["bg"], bg), "bck sums"
    assert same_bits(r["dx"], bn_ref.bck_in_np(r["x"], mean, istd, r["scale"], sg, bg, r["dy"])), "dx"


def big_term_inputs():
    """One channel, T = 2, HW = 3, dy = [2^24, 1, 1 | 1, 1, 1].  One chunk: chain 0 owns elements 0 .. 3 and 2^24 swallows its three 1s one by one, chain 1 holds 1 + 1,
    the tree gives 2^24 + 2 = 16777218.  Two chunks: the first chunk's total is 2^24 (two 1s swallowed), the second's is 3, and 2^24 + 3 rounds to even: 16777220.
    x is anything with a finite inv_std."""
    dy = np.array([[[[2.0 ** 24, 1, 1]]], [[[1, 1, 1]]]], F)
    x = np.array([[[[0.5, -1.0, 2.0]]], [[[1.5, -0.25, 0.75]]]], F)
    return x, dy
