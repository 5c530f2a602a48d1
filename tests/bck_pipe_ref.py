"""numpy restatements for the full-net gradient pipe (DESIGN.md sections 3.11 - 3.13), written from the semantics, not from the backend.

  * the four plumbing functions in fp32, bit for bit: reduce_f32, dropout_f32 (the hash in uint32, the float threshold, the double-then-float scale), concat_f32, split_f32
  * net_f64: a float64 forward plus backprop of a ConvPipe capped with softmax losses -- convolution, ReLU, max / average pooling, LRN, dropout with the SAME mask, concat,
    sums at fan-outs.  It walks the forward ops backwards and ACCUMULATES into one gradient per node, so it shares neither names nor order with add_bck_ops.
    It also guards the comparison: a tolerance as loose as 5e-4 would pass a flipped ReLU or argmax, so no ReLU input may lie within 1e-4 max|v| of zero and no pooling
    window's two largest values within 1e-4 max|v| of each other (net_f64 raises otherwise; the tests pick seeds for which it does not)."""
import numpy as np

U = 2.0 ** -24


# ---- the four functions, fp32
def reduce_f32(ins):
    v = np.zeros_like(np.asarray(ins[0], np.float32))   # +0
    for x in ins:
        v = (v + np.asarray(x, np.float32)).astype(np.float32)
    return v


def dropout_hash(n, seed):
    with np.errstate(over="ignore"):
        h = (np.arange(n, dtype=np.uint64) + np.uint64(seed)).astype(np.uint32)   # wraps
        h ^= h >> np.uint32(16); h *= np.uint32(0x85ebca6b); h ^= h >> np.uint32(13); h *= np.uint32(0xc2b2ae35); h ^= h >> np.uint32(16)
    return h


def dropout_seed_hitting(ratio, index):
    """The seed under which element `index` hashes to EXACTLY the threshold (the mix is a bijection of uint32, inverted step by step): that element is dropped by the
    template's `>` and would be kept by `>=`."""
    M = 1 << 32
    h = int(dropout_thresh(ratio))
    h ^= h >> 16
    h = (h * pow(0xc2b2ae35, -1, M)) % M
    h ^= h >> 13; h ^= h >> 26
    h = (h * pow(0x85ebca6b, -1, M)) % M
    h ^= h >> 16
    return (h - index) % M


def dropout_thresh(ratio):
    return np.uint32(int(np.float32(4294967296.0) * np.float32(ratio)))   # (float)0xffffffff is 2^32; a float product, truncated


def dropout_scale(ratio):
    return np.float32(1.0 / (1.0 - float(np.float32(ratio))))


def dropout_keep(n, ratio, seed):
    return dropout_hash(n, seed) > dropout_thresh(ratio)


def dropout_f32(x, ratio, seed):
    x = np.asarray(x, np.float32)
    keep = dropout_keep(x.size, ratio, seed).reshape(x.shape)
    return np.where(keep, (x * dropout_scale(ratio)).astype(np.float32), np.float32(0.0)).astype(np.float32)


def concat_f32(ins):
    return np.concatenate([np.asarray(x, np.float32) for x in ins], axis=1)


def split_f32(x, chans):
    outs, c0 = [], 0
    for c in chans:
        outs.append(np.ascontiguousarray(x[:, c0:c0 + c])); c0 += c
    return outs


# ---- float64 layers
def conv_f64(x, f, b, stride, pad):
    B, C, H, W = x.shape; OC, _, KH, KW = f.shape
    OH, OW = (H + 2 * pad[0] - KH) // stride[0] + 1, (W + 2 * pad[1] - KW) // stride[1] + 1
    xp = np.zeros((B, C, H + 2 * pad[0], W + 2 * pad[1])); xp[:, :, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x
    out = np.zeros((B, OC, OH, OW))
    for ky in range(KH):
        for kx in range(KW):
            out += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + OH * stride[0]:stride[0], kx:kx + OW * stride[1]:stride[1]][:, :, :OH, :OW], f[:, :, ky, kx])
    return out + b.reshape(1, OC, 1, 1)


def conv_bck_f64(x, f, og, stride, pad):
    B, C, H, W = x.shape; OC, _, KH, KW = f.shape; OH, OW = og.shape[2:]
    xp = np.zeros((B, C, H + 2 * pad[0], W + 2 * pad[1])); xp[:, :, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = x
    gxp = np.zeros_like(xp); gf = np.zeros_like(f, dtype=np.float64)
    for ky in range(KH):
        for kx in range(KW):
            sl = (slice(None), slice(None), slice(ky, ky + OH * stride[0], stride[0]), slice(kx, kx + OW * stride[1], stride[1]))
            gf[:, :, ky, kx] = np.einsum("bchw,bohw->oc", xp[sl][:, :, :OH, :OW], og)
            gxp[sl][:, :, :OH, :OW] += np.einsum("bohw,oc->bchw", og, f[:, :, ky, kx])
    return gxp[:, :, pad[0]:pad[0] + H, pad[1]:pad[1] + W], gf, og.sum(axis=(0, 2, 3))


def pool_windows(H, W, OH, OW, kern, stride, pad):
    for oy in range(OH):
        for ox in range(OW):
            taps = [(oy * stride[0] + ky - pad[0], ox * stride[1] + kx - pad[1]) for kx in range(kern[1]) for ky in range(kern[0])]   # kx outer, ky inner
            yield oy, ox, [(y, x) for y, x in taps if 0 <= y < H and 0 <= x < W]


def pool_f64(x, out_hw, kern, stride, pad, avg, guard):
    """-> out, and per output the winning tap (max).  Average: the taps inside the plane divided by their number."""
    B, C, H, W = x.shape; OH, OW = out_hw
    out = np.zeros((B, C, OH, OW)); arg = np.full((B, C, OH, OW, 2), -1, int)
    for oy, ox, taps in pool_windows(H, W, OH, OW, kern, stride, pad):
        v = np.stack([x[:, :, y, xx] for y, xx in taps], axis=-1)
        if avg:
            out[:, :, oy, ox] = v.sum(axis=-1) / len(taps)
            continue
        i = v.argmax(axis=-1)
        out[:, :, oy, ox] = v.max(axis=-1)
        arg[:, :, oy, ox] = np.array(taps)[i]
        if len(taps) > 1:
            s = np.sort(v, axis=-1)
            if np.min(s[..., -1] - s[..., -2]) < guard:
                raise AssertionError("net_f64 guard: a pooling window's two largest values are too close for a 5e-4 comparison to notice a flipped argmax")
    return out, arg


def pool_bck_f64(x_shape, og, arg, kern, stride, pad, avg):
    """max: the gradient goes to the winning tap; average: og / (KH * KW) to every tap inside the plane -- the FULL window area, also where a border clips the window."""
    B, C, H, W = x_shape; OH, OW = og.shape[2:]
    g = np.zeros(x_shape)
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing="ij")
    for oy, ox, taps in pool_windows(H, W, OH, OW, kern, stride, pad):
        if avg:
            for y, xx in taps:
                g[:, :, y, xx] += og[:, :, oy, ox] / (kern[0] * kern[1])
        else:
            np.add.at(g, (bi, ci, arg[:, :, oy, ox, 0], arg[:, :, oy, ox, 1]), og[:, :, oy, ox])
    return g


def lrn_f64(x, ls, alpha, beta, k):
    C = x.shape[1]; h = ls // 2
    sq = np.zeros_like(x)
    for c in range(C):
        sq[:, c] = (x[:, max(0, c - h):min(C, c + h + 1)] ** 2).sum(axis=1)
    sb = k + sq * (alpha / ls)
    return x * sb ** -beta, sb


def lrn_bck_f64(x, out, sb, og, ls, alpha, beta):
    C = x.shape[1]; h = ls // 2
    t = og * out / sb
    ts = np.zeros_like(x)
    for c in range(C):
        ts[:, c] = t[:, max(0, c - h):min(C, c + h + 1)].sum(axis=1)
    return og * sb ** -beta + x * ts * (-2.0 * beta * alpha / ls)


def net_f64(cp, loss_tops, params, data, label, drop_seeds, ratio=0.5, guard_rel=1e-4):
    """Forward and backprop of ConvPipe `cp` in float64.  loss_tops: the nodes capped with a softmax loss (label shared); drop_seeds: Dropout op tag -> the uint32 seed
    of its mask.  -> {<node>_grad_loss, <param>_grad_loss, loss names ('loss', or 'loss1' ... in order)}: each <node>_grad_loss is the gradient with respect to the
    node's value BEFORE its in-place ops, which is what the pipe leaves in that var."""
    f64 = lambda a: np.asarray(a, np.float64)
    val = {cp.in_node: f64(data)}
    keep = {}   # per op tag: what the backward pass needs
    for o in cp.ops:
        x = val[o.bot]
        if o.type == "Convolution":
            keep[o.tag] = x
            val[o.top] = conv_f64(x, f64(params[o.tag + "_filts"]), f64(params[o.tag + "_biases"]), o.stride, o.in_pad)
        elif o.type == "ReLU":
            if np.min(np.abs(x)) < guard_rel * np.max(np.abs(x)):
                raise AssertionError(f"net_f64 guard: ReLU {o.tag} has an input within {guard_rel} max|v| of zero")
            keep[o.tag] = x > 0
            val[o.top] = np.where(x > 0, x, 0.0)
        elif o.type == "Pooling":
            d = cp.nodes[o.top]
            out, arg = pool_f64(x, (d.dsz("y"), d.dsz("x")), o.kern_sz, o.stride, o.in_pad, o.avg_pool, guard_rel * np.max(np.abs(x)))
            keep[o.tag] = (x.shape, arg); val[o.top] = out
        elif o.type == "LRN":
            ls, alpha, beta, k = o.lrn
            out, sb = lrn_f64(x, ls, float(np.float32(alpha)), float(np.float32(beta)), float(np.float32(k)))
            keep[o.tag] = (x, out, sb); val[o.top] = out
        elif o.type == "Dropout":
            m = dropout_keep(x.size, ratio, drop_seeds[o.tag]).reshape(x.shape) * float(dropout_scale(ratio))
            keep[o.tag] = m; val[o.top] = x * m
        elif o.type == "Concat":
            val[o.top] = np.concatenate([val[b] for b in o.bots], axis=1)
        else:
            raise AssertionError(o.type)
    res, grad = {}, {}
    B = data.shape[0]
    lab = np.asarray(label).reshape(B).astype(int)
    for i, t in enumerate(loss_tops):
        z = val[t].reshape(B, -1)
        e = np.exp(z - z.max(axis=1, keepdims=True)); p = e / e.sum(axis=1, keepdims=True)
        res["loss" if len(loss_tops) == 1 else f"loss{i + 1}"] = float(-np.log(p[np.arange(B), lab]).mean())
        p[np.arange(B), lab] -= 1.0
        grad[t] = grad.get(t, 0.0) + (p / B).reshape(val[t].shape)
    for o in reversed(cp.ops):
        og = grad[o.top]
        if o.type == "Convolution":
            gx, gf, gb = conv_bck_f64(keep[o.tag], f64(params[o.tag + "_filts"]), og, o.stride, o.in_pad)
            res[o.tag + "_filts_grad_loss"] = gf; res[o.tag + "_biases_grad_loss"] = gb
            grad[o.bot] = grad.get(o.bot, 0.0) + gx
        elif o.type == "ReLU":
            grad[o.top] = np.where(keep[o.tag], og, 0.0)
        elif o.type == "Dropout":
            grad[o.top] = og * keep[o.tag]
        elif o.type == "Pooling":
            shp, arg = keep[o.tag]
            grad[o.bot] = grad.get(o.bot, 0.0) + pool_bck_f64(shp, og, arg, o.kern_sz, o.stride, o.in_pad, o.avg_pool)
        elif o.type == "LRN":
            x, out, sb = keep[o.tag]; ls, alpha, beta, k = o.lrn
            grad[o.bot] = grad.get(o.bot, 0.0) + lrn_bck_f64(x, out, sb, og, ls, float(np.float32(alpha)), float(np.float32(beta)))
        elif o.type == "Concat":
            c0 = 0
            for b in o.bots:
                c = cp.nodes[b].dsz("chan")
                grad[b] = grad.get(b, 0.0) + og[:, c0:c0 + c]; c0 += c
    for n, g in grad.items():
        res[n + "_grad_loss"] = g
    return res


def rel_err(got, want):
    """max|got - want| / max|want|: the reference's own measure for its gradient pipes."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64).reshape(want.shape) - want)) / max(np.max(np.abs(want)), 1e-300))
