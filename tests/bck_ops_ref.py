"""Not a test: a numpy restatement of the semantics of the gradient pipe's non-conv functions (the header of
boda_amd/csrc/kernels/bck_ops_f32.hip), used by tests/test_bck_ops_cpu.py and tests/test_gpu_bck_ops.py.

Every `*_f32` function computes in np.float32, one rounding per written operation, in the element order the semantics give (the loops run over the window / channel /
image index; the independent outputs are numpy axes).  powf / expf / logf are the C library's own (the ones be=cpu links), called through ctypes: numpy's float32
pow / exp / log are separate implementations that round differently.  Every `*_f64` function is the same formula in float64 on the same fp32 inputs: the reference of
the bounded outputs."""
import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
U = 2.0 ** -24   # unit roundoff of fp32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _na in (("powf", 2), ("expf", 1), ("logf", 1)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _na


def _map(fn, *arrs):
    arrs = np.broadcast_arrays(*[np.asarray(a, f32) for a in arrs])
    out = np.empty(arrs[0].shape, f32)
    flat = [a.reshape(-1) for a in arrs]
    o = out.reshape(-1)
    for i in range(o.size):
        o[i] = fn(*[float(a[i]) for a in flat])
    return out


def powf(a, b): return _map(_libm.powf, a, b)
def expf(a): return _map(_libm.expf, a)
def logf(a): return _map(_libm.logf, a)


def pool_out_sz(in_sz, k, s, p):
    pin = in_sz + 2 * p
    return 1 if pin < k else -(-(pin - k) // s) + 1


def pool_yx_f32(x, kern, stride, pad):
    """-> (out, out_in_yx).  Max pooling; taps kx outer, ky inner; strict > from -FLT_MAX (the first maximal tap wins); out_in_yx = float(in_y*W + in_x) or -1."""
    x = np.asarray(x, f32); B, C, H, W = x.shape
    (KH, KW), (SY, SX), (PY, PX) = kern, stride, pad
    OH, OW = pool_out_sz(H, KH, SY, PY), pool_out_sz(W, KW, SX, PX)
    if H + 2 * PY < KH or W + 2 * PX < KW:   # either padded dim below the window: the op's out plane is 1 x 1
        OH = OW = 1
    out = np.full((B, C, OH, OW), -FLT_MAX, f32); yx = np.full((B, C, OH, OW), -1.0, f32)
    for oy in range(OH):
        for ox in range(OW):
            for kx in range(KW):
                for ky in range(KH):
                    iy, ix = oy * SY + ky - PY, ox * SX + kx - PX
                    if iy < 0 or ix < 0 or ix >= W or iy >= H:
                        continue
                    v = x[:, :, iy, ix]
                    m = v > out[:, :, oy, ox]
                    out[:, :, oy, ox] = np.where(m, v, out[:, :, oy, ox])
                    yx[:, :, oy, ox] = np.where(m, f32(iy * W + ix), yx[:, :, oy, ox])
    return out, yx


def spreading_f32(ogl, out_in_yx, in_hw, kern, stride, pad, avg):
    """-> in_grad_loss.  Per input pel: candidate outputs out_x outer, out_y inner; sequential fp32 sum from +0; max: where out_in_yx == y*W + x;
    average: out_grad_loss / (KH*KW), the full area also at clipped borders."""
    ogl = np.asarray(ogl, f32); B, C, OH, OW = ogl.shape
    H, W = in_hw
    (KH, KW), (SY, SX), (PY, PX) = kern, stride, pad
    igl = np.zeros((B, C, H, W), f32)
    area = f32(KH * KW)
    for y in range(H):
        for x in range(W):
            oxb, oxe = max(0, x + PX - KW + SX) // SX, min((x + PX) // SX + 1, OW)
            oyb, oye = max(0, y + PY - KH + SY) // SY, min((y + PY) // SY + 1, OH)
            v = np.zeros((B, C), f32)
            for ox in range(oxb, oxe):
                for oy in range(oyb, oye):
                    if avg:
                        v = v + ogl[:, :, oy, ox] / area
                    else:
                        v = np.where(out_in_yx[:, :, oy, ox] == f32(y * W + x), v + ogl[:, :, oy, ox], v)
            igl[:, :, y, x] = v
    return igl


def lrn_sb_f32(x, local_size, alpha, beta, k):
    """-> (out, out_scale_base).  ls_sum carried as (ls_sum + new^2) - old^2; scale_base = k + ls_sum * (alpha / local_size); out = in * powf(scale_base, -beta)."""
    x = np.asarray(x, f32); B, C, H, W = x.shape
    h = local_size // 2
    aol = f32(alpha) / f32(local_size)
    sb = np.empty_like(x)
    ls_sum = np.zeros((B, H, W), f32)
    zero = np.zeros((B, H, W), f32)
    for c in range(C + h):
        new = x[:, c] if c < C else zero
        old = x[:, c - local_size] if 0 <= c - local_size < C else zero
        ls_sum = ls_sum + new * new
        ls_sum = ls_sum - old * old
        if c >= h:
            sb[:, c - h] = f32(k) + ls_sum * aol
    return x * powf(sb, -f32(beta)), sb


def lrn_out_f64(x, sb, beta):
    return np.asarray(x, np.float64) * np.asarray(sb, np.float64) ** -float(f32(beta))


def _bck_lrn_terms(out, ogl, sb, local_size, dt):
    """t[c] = ogl*out/sb and, per channel, the window's terms in ring-slot order (slot = channel mod local_size), zeros outside the tensor."""
    t = (np.asarray(ogl, dt) * np.asarray(out, dt)) / np.asarray(sb, dt)
    C = t.shape[1]; h = local_size // 2
    zero = np.zeros_like(t[:, 0])
    for c in range(C):
        chans = sorted(range(c - h, c + h + 1), key=lambda ch: ch % local_size)
        yield c, [t[:, ch] if 0 <= ch < C else zero for ch in chans]


def bck_lrn_f32(x, out, ogl, sb, local_size, alpha, beta, k):
    x, out, ogl, sb = (np.asarray(a, f32) for a in (x, out, ogl, sb))
    coef = ((f32(2.0) * -f32(beta)) * f32(alpha)) / f32(local_size)
    a = ogl * powf(sb, -f32(beta))
    igl = np.empty_like(x)
    for c, terms in _bck_lrn_terms(out, ogl, sb, local_size, f32):
        ls_sum = np.zeros_like(x[:, 0])
        for t in terms:
            ls_sum = ls_sum + t
        igl[:, c] = a[:, c] + x[:, c] * ls_sum * coef
    return igl


def bck_lrn_f64(x, out, ogl, sb, local_size, alpha, beta, k):
    """-> (want, S): the float64 formula and the magnitude S = |ogl * sb^-beta| + |in| * sum|t| * |2 beta alpha / local_size| its error bound scales with."""
    x, out, ogl, sb = (np.asarray(a, np.float64) for a in (x, out, ogl, sb))
    al, be = float(f32(alpha)), float(f32(beta))
    coef = 2.0 * -be * al / local_size
    a = ogl * sb ** -be
    want = np.empty_like(x); S = np.empty_like(x)
    for c, terms in _bck_lrn_terms(out, ogl, sb, local_size, np.float64):
        want[:, c] = a[:, c] + x[:, c] * sum(terms) * coef
        S[:, c] = np.abs(a[:, c]) + np.abs(x[:, c]) * sum(np.abs(t) for t in terms) * abs(coef)
    return want, S


def zero_if_non_pos_f32(x, cond):
    return np.where(np.asarray(cond, f32) > 0, np.asarray(x, f32), f32(0.0))


def softmax_f32(x):
    """in img:chan:1:1.  pel_max starts at 0; prob = expf(in - pel_max) / (sequential sum over the channels)."""
    x = np.asarray(x, f32); B, C = x.shape[:2]
    xr = x.reshape(B, C)
    pel_max = np.maximum(f32(0.0), xr.max(axis=1))
    e = expf(xr - pel_max[:, None])
    s = np.zeros(B, f32)
    for c in range(C):
        s = s + e[:, c]
    return (e / s[:, None]).reshape(x.shape)


def softmax_f64(x):
    xr = np.asarray(x, np.float64).reshape(x.shape[0], x.shape[1])
    e = np.exp(xr - np.maximum(0.0, xr.max(axis=1))[:, None])
    return (e / e.sum(axis=1)[:, None]).reshape(x.shape)


def sm_grad_and_loss_f32(prob, label):
    """-> (in_grad_loss, loss_per_pel): (prob - [chan == label]) / img_count (subtract, then divide); -logf(max(prob[label], FLT_MIN))."""
    prob = np.asarray(prob, f32); B, C = prob.shape[:2]
    pr = prob.reshape(B, C); lab = np.asarray(label, f32).reshape(B).astype(np.int64)
    v = pr.copy()
    v[np.arange(B), lab] = v[np.arange(B), lab] - f32(1.0)
    v = v / f32(B)
    loss = -logf(np.maximum(pr[np.arange(B), lab], FLT_MIN))
    return v.reshape(prob.shape), loss.reshape(B, 1, 1)


def loss_per_pel_f64(prob, label):
    B, C = prob.shape[:2]
    pr = np.asarray(prob, np.float64).reshape(B, C); lab = np.asarray(label).reshape(B).astype(np.int64)
    return (-np.log(np.maximum(pr[np.arange(B), lab], float(FLT_MIN)))).reshape(B, 1, 1)


def sum_loss_over_imgs_f32(loss_per_pel):
    l = np.asarray(loss_per_pel, f32).reshape(-1)
    v = f32(0.0)
    for i in range(l.size):
        v = f32(v + l[i])
    return np.array([[v / f32(l.size)]], f32)
