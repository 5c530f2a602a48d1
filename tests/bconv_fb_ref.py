"""The exact fp32 chains of hip_bconv_filts_biases on be=hip (boda_amd/csrc/kernels/bconv_fb_f32.hip), rebuilt in numpy: what the tests hold the kernel to.

Filter gradient: oracle.bck_chain.filts_chain(in, out_grad_loss, geom, BK, KSL) -- imported, not copied: slab s = one ascending-k fma chain from +0 over the K range
of slice s, the slabs added in slice order.

Bias gradient (biases_chain below), as the kernel's header writes it: with k = (img, oy, ox) ascending and I(k, oc) = out_grad_loss[img, oc, oy, ox], per slice and
out_chan there are BK chains, one per residue a = k % BK:  c_a = sum_t I(t*BK + a, oc)  over the slice's K steps t in ascending order, from +0, plain fp32 adds, a
term past K being +0.  The slice's partial is ((c_0 + c_1) + c_2) + ... + c_{BK-1}; an empty slice's is +0.  The partials are added in slice order,
partial[0] + partial[1] + ... + partial[KSL-1].  The slice ranges are bck_chain.filts_slices(K, BK, KSL): whole K steps, so every slice starts at residue 0."""
import numpy as np

from oracle import bck_chain as bc
from oracle.bck_chain import filts_chain   # noqa: F401  (the filter chain, for the tests that import this module)

f32 = np.float32

# the shapes both test files run: (B, C, H = W, OC, k, stride, pad)
SHAPES = {
    "k1_ohw49_tail": (3, 20, 7, 24, 1, 1, 0),       # OH*OW = 49: no 4-element alignment; K = 147 with a tail at every K step depth
    "k1_ohw64_ragged": (2, 68, 8, 40, 1, 1, 0),     # OH*OW % 4 == 0, ragged channels
    "k1_stride2": (2, 16, 9, 12, 1, 2, 0),          # the strided 1x1
    "k3_borders": (2, 5, 6, 7, 3, 1, 1),
    "k7_stem": (1, 3, 17, 9, 7, 2, 3),
    "k1_many_tiles": (2, 130, 6, 70, 1, 1, 0),      # several tiles both ways at 64 x 64 tiles
    "k1_long_k": (4, 8, 28, 8, 1, 1, 0),            # K = 3136 on one tile: the planner slices it
}
PLANS = [(32, 1), (32, 40), (16, 7), (32, 98)]      # (BK, KSL) pairs of the float64 checks


def shape_op(name):
    from test_bck_conv_cpu import bck_op
    B, C, H, OC, k, s, p = SHAPES[name]
    return bck_op(B, C, H, H, OC, k, k, s, s, p, p)


def plan_of(launch):
    """(BK, KSL) of a bodahip_bconv_filts_biases launch, from its configuration string BIxBJxBK_wWIxWJ[_sKSL]."""
    assert launch["kernel"] == "bodahip_bconv_filts_biases", launch
    cfg = launch["cfg"]
    return int(cfg.split("_")[0].split("x")[2]), (int(cfg.split("_s")[1].split("_")[0]) if "_s" in cfg else 1)


def biases_chain(g, BK, KSL):
    """biases_grad_loss[OC] of out_grad_loss g[img, oc, oy, ox] under (BK, KSL)."""
    g = np.asarray(g, f32)
    B, OC = g.shape[:2]
    I = np.ascontiguousarray(g.reshape(B, OC, -1).transpose(0, 2, 1)).reshape(-1, OC)   # [K, OC], k = (img, oy, ox)
    K = I.shape[0]
    total = None
    for k0, k1 in bc.filts_slices(K, BK, KSL):
        c = np.zeros((BK, OC), f32)                       # the BK chains of every out_chan
        for t0 in range(k0, k1, BK):
            step = np.zeros((BK, OC), f32)                # one K step; rows past K stay +0
            step[:min(BK, K - t0)] = I[t0:t0 + BK]
            c = c + step
        part = c[0]
        for a in range(1, BK):
            part = part + c[a]
        total = part if total is None else total + part
    return np.ascontiguousarray(total, f32)
