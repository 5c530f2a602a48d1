"""The exact fp32 chains of the BckConv gradient kernels, rebuilt on the CPU (TEST INFRASTRUCTURE ONLY, like boda_oracle).

numpy index arithmetic + the oracle's sgemm (an ascending-k fmaf chain from +0 per output: the arithmetic of v_mfma_f32_32x32x2_f32).  Every function follows the
association WRITTEN DOWN in a kernel's header (boda_amd/csrc/kernels/bconv_filts_f32.hip, bconv_in_f32.hip) and asks nothing of the code under test: tile depth
and slice count are inputs.  `geom` is Op.bck_conv_geom(): B C H W OC KH KW SY SX PY PX OH OW (the forward convolution's geometry).

The operands are plain gathers with +0.0 where the kernels read out of bounds; a zero term is fma(a, 0, acc) = acc for finite data as long as acc is not -0, so the
zero-padded chains carry the bits of the chains without those terms -- up to the sign of a zero: an accumulator becomes -0 when a negative product underflows
(fma(a, b, +0) rounds to -0), and a padded term fma(+0, w, -0) with w > 0 makes it +0 again.  The K tail does the same: a kernel runs whole K steps of BK terms, and
the terms past K are fma(+0, +0, acc), which turn a -0 into +0 and change nothing else.  filts_sliced_chain forms them where a slice ends in a partial K step;
in_grad_chain forms them when it is given the K step `bk` of the launch.
"""
from __future__ import annotations
import numpy as np

from . import boda_oracle as bo

f32 = np.float32


def filts_operands(x, g, geom):
    """-> (I[K, OC], J[K, C*KH*KW]): I[k, oc] = out_grad_loss[img, oc, oy, ox], J[k, (c, fy, fx)] = in[img, c, oy*SY - PY + fy, ox*SX - PX + fx] or +0.0 outside the
    plane; k = (img, oy, ox) ascending."""
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX, OH, OW = (geom[k] for k in ("B", "C", "H", "W", "OC", "KH", "KW", "SY", "SX", "PY", "PX", "OH", "OW"))
    x = np.asarray(x, f32).reshape(B, C, H, W); g = np.asarray(g, f32).reshape(B, OC, OH, OW)
    K = B * OH * OW
    I = np.ascontiguousarray(g.transpose(0, 2, 3, 1)).reshape(K, OC)
    # rows / columns each tap reads: iy[fy, oy], ix[fx, ox]; anything outside the plane is a zero
    xp = np.zeros((B, C, H + 1, W + 1), f32); xp[:, :, :H, :W] = x   # row H / column W: the zero every out-of-plane read is sent to
    iy = np.arange(OH)[None, :] * SY - PY + np.arange(KH)[:, None]
    ix = np.arange(OW)[None, :] * SX - PX + np.arange(KW)[:, None]
    iy = np.where((iy >= 0) & (iy < H), iy, H); ix = np.where((ix >= 0) & (ix < W), ix, W)
    pat = xp[:, :, iy[:, :, None, None], ix[None, None, :, :]]       # (B, C, KH, OH, KW, OW)
    J = np.ascontiguousarray(pat.transpose(0, 3, 5, 1, 2, 4)).reshape(K, C * KH * KW)
    return I, J


def filts_slices(K, BK, KSL):
    """The K ranges [k0, k1) of the KSL slices: nkt = ceil(K / BK) K steps, kt_per = ceil(nkt / KSL) per slice, clipped to nkt and then to K (k0 == k1: empty)."""
    nkt = -(-K // BK); kt_per = -(-nkt // KSL)
    out = []
    for s in range(KSL):
        kt0 = min(s * kt_per, nkt); kt1 = min(kt0 + kt_per, nkt)
        out.append((min(kt0 * BK, K), min(kt1 * BK, K)))
    return out


def filts_sliced_chain(I, J, BK, KSL, dims=None):
    """The filter gradient as bodahip_bconv_filts associates it: slab s = one fmaf chain from +0 over the K range of slice s (an empty slice: +0.0), then
    slab[0] + slab[1] + ... + slab[KSL-1] in slice order as fp32 additions.  -> [OC, C*KH*KW], or reshaped to `dims` (OC, C, KH, KW)."""
    K, OC = I.shape
    assert J.shape[0] == K and BK >= 1 and KSL >= 1
    acc = None
    for k0, k1 in filts_slices(K, BK, KSL):
        slab = bo.sgemm(I[k0:k1], J[k0:k1]) if k1 > k0 else np.zeros((OC, J.shape[1]), f32)
        if (k1 - k0) % BK:   # the slice ends in the K tail: fma(+0, +0, acc) terms (a -0 becomes +0, a NaN stays)
            slab = slab + f32(0.0)
        with np.errstate(invalid="ignore", over="ignore"):   # (slabs that overflow, slabs of +Inf and -Inf: the Inf and the NaN are the kernel's too)
            acc = slab if acc is None else (acc + slab).astype(f32, copy=False)
    return acc.reshape(dims) if dims is not None else acc


def filts_chain(x, g, geom, BK, KSL):
    """filts_grad_loss[OC, C, KH, KW] for given tensors: filts_operands + filts_sliced_chain."""
    I, J = filts_operands(x, g, geom)
    return filts_sliced_chain(I, J, BK, KSL, (geom["OC"], geom["C"], geom["KH"], geom["KW"]))


def biases_chain(g):
    """The bias gradient as bodahip_bconv_biases (-DBIAS_ONLY) sums it: per out_chan, thread t of 256 adds the elements e = t, t + 256, ... of the flat (img, pel)
    sequence to a +0 start, then the tree red[t] += red[t + h] for h = 128 ... 1.  g = out_grad_loss[img, oc, oy, ox] -> [OC]."""
    g = np.asarray(g, f32)
    B, OC = g.shape[:2]
    a = np.ascontiguousarray(g.reshape(B, OC, -1).transpose(1, 0, 2)).reshape(OC, -1)
    n = a.shape[1]
    red = np.zeros((OC, 256), f32)
    for e0 in range(0, n, 256):
        m = min(256, n - e0)   # the tail: only the first m threads have an element left
        red[:, :m] = red[:, :m] + a[:, e0:e0 + m]
    h = 128
    while h:
        red[:, :h] = red[:, :h] + red[:, h:2 * h]
        h >>= 1
    return red[:, 0].copy()


def in_grad_chain(w, g, geom, bk=0):
    """The data gradient as ONE chain per output in the reference template's order: k = (out_chan, out_x, out_y) ascending, the filter taps descending with them.
    Per phase (ry, rx) = ((y + PY) % SY, (x + PX) % SX) every pel meets the same TY x TX window of taps: out position (qy - (TY-1) + ty, qx - (TX-1) + tx) with
    q = (pel + pad) / stride, tap (ry + SY*(TY-1-ty), rx + SX*(TX-1-tx)).  Explicit operands with +0.0 where the out position or the tap does not exist, one
    oracle sgemm per phase and image.  bk: the K step of the launch; where OC * TY * TX is no multiple of it the chain ends in K-tail terms fma(+0, +0, acc).
    w = filts[OC, C, KH, KW], g = out_grad_loss[B, OC, OH, OW] -> in_grad_loss[B, C, H, W]."""
    B, C, H, W, OC, KH, KW, SY, SX, PY, PX, OH, OW = (geom[k] for k in ("B", "C", "H", "W", "OC", "KH", "KW", "SY", "SX", "PY", "PX", "OH", "OW"))
    w = np.asarray(w, f32).reshape(OC, C, KH, KW); g = np.asarray(g, f32).reshape(B, OC, OH, OW)
    TY, TX = -(-KH // SY), -(-KW // SX)
    wz = np.zeros((OC, C, KH + 1, KW + 1), f32); wz[:, :, :KH, :KW] = w       # tap row KH / column KW: zero
    gz = np.zeros((B, OC, OH + 1, OW + 1), f32); gz[:, :, :OH, :OW] = g       # out row OH / column OW: zero
    out = np.zeros((B, C, H, W), f32)
    for ry in range(SY):
        ys = np.array([y for y in range(H) if (y + PY) % SY == ry], np.int64)
        fy = ry + SY * (TY - 1 - np.arange(TY)); fy = np.where(fy < KH, fy, KH)
        for rx in range(SX):
            xs = np.array([x for x in range(W) if (x + PX) % SX == rx], np.int64)
            if not len(ys) or not len(xs):
                continue
            fx = rx + SX * (TX - 1 - np.arange(TX)); fx = np.where(fx < KW, fx, KW)
            wp = wz[:, :, fy[None, :], fx[:, None]]                            # (OC, C, TX, TY)
            a = np.ascontiguousarray(wp.transpose(0, 2, 3, 1)).reshape(OC * TX * TY, C)
            oy = (ys + PY) // SY - (TY - 1) + np.arange(TY)[:, None]           # (TY, ny)
            ox = (xs + PX) // SX - (TX - 1) + np.arange(TX)[:, None]           # (TX, nx)
            oy = np.where((oy >= 0) & (oy < OH), oy, OH); ox = np.where((ox >= 0) & (ox < OW), ox, OW)
            for img in range(B):
                gp = gz[img][:, oy[None, :, :, None], ox[:, None, None, :]]    # (OC, TX, TY, ny, nx)
                r = bo.sgemm(a, np.ascontiguousarray(gp).reshape(OC * TX * TY, len(ys) * len(xs)))
                if bk and (OC * TX * TY) % bk:
                    r = r + f32(0.0)
                out[img][:, ys[:, None], xs[None, :]] = r.reshape(C, len(ys), len(xs))
    return out
