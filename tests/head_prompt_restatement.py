"""Kernel-blind restatements of the glue ops of the PromptIR prompt block and of the degradation-classifier head, in plain torch on the
CPU, written from the statements in the headers of promptir.hip / dchead.hip and the reference lines they cite.  Nothing here imports the
package under test.

    prompt_mix          bilinear_(S,S)->(H,W)( sum_l softmax(logits)[b, l] * param[l] )
    meanpool_fc         mean over the pixels -> Linear
    conv1x1_pool_relu   Conv2d(1x1, no bias) -> MaxPool2d(2, 2) -> ReLU
    mix                 prev + softmax(mixing_weights)[idx] * feat
    conv_embed_ln       Conv2d(k, stride, pad) + bias -> channels-first LayerNorm (eps 1e-6)

Every function returns ``(outs, n)``: ``outs`` maps a name to the forward value / the gradient of that input (gradients from torch
autograd, present when the incoming gradient is given), ``n`` maps the same names to the length of the longest chain of additions an
element of that output passes through (nested sums add their lengths; an upper bound).

``dtype``: the arithmetic of the expression, float64 by default.  float32 gives the same expression in torch's CPU fp32, the yardstick of
what rounding alone does to it.

``absolute=True`` gives, under the same names, the magnitude sum A of each output element: the same expression on the absolute values of
all inputs, weights and incoming gradients, so that no term cancels another.  What only scales or selects is taken from the signed run:
the softmax weights, the max-pool routing and ReLU mask, the LayerNorm's 1 / sigma.  Differences become sums (x - mean -> |x| + mean |x|,
delta_ij - s_j -> delta_ij + s_j)."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24      # unit roundoff of fp32


def _leaf(t, dtype, absolute=False):
    t = t.detach().to(dtype)
    return (t.abs() if absolute else t.clone()).requires_grad_(True)


def softmax(x, dim=-1):
    """with the maximum subtracted, in x's own dtype"""
    e = torch.exp(x - x.max(dim=dim, keepdim=True).values)
    return e / e.sum(dim=dim, keepdim=True)


# ---- prompt mix ----------------------------------------------------------------------------------------------------------------
def lerp_taps(S, n_dst, fused=False):
    """F.interpolate(mode="bilinear", align_corners=False) along one axis, S -> n_dst: (i0, i1, l0, l1) per destination index.  The source
    coordinate and the two weights are float32, as promptir.hip states them: src = (S / n_dst) * (dst + 0.5) - 0.5 clamped at 0,
    i0 = floor(src), i1 = min(i0 + 1, S - 1), weights (1 - l, l) with l = src - i0.  float32 arithmetic has two evaluations of src: the
    product rounded before the subtraction, or (``fused``) both in one FMA with a single rounding, which is what a compiler that
    contracts a * b - c gives.  They differ by an ulp of src in some rows, at S = 32 by up to 2^-19."""
    dst = np.arange(n_dst, dtype=np.float32)
    scale = np.float32(S) / np.float32(n_dst)
    if fused:   # (the product of two float32 numbers is exact in float64, and so is the subtraction of 0.5: one rounding)
        src = (scale.astype(np.float64) * (dst + np.float32(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    else:
        src = scale * (dst + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0.0))
    i0 = np.minimum(np.floor(src).astype(np.int64), S - 1)
    i1 = np.minimum(i0 + 1, S - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1.0) - l1
    assert src.dtype == l0.dtype == l1.dtype == np.float32
    return i0, i1, l0, l1


def lerp_matrix(S, n_dst, fused=False):
    """the dense (n_dst, S) interpolation matrix of lerp_taps, the float32 weights widened to float64"""
    i0, i1, l0, l1 = lerp_taps(S, n_dst, fused)
    R = np.zeros((n_dst, S), dtype=np.float64)
    rows = np.arange(n_dst)
    np.add.at(R, (rows, i0), l0.astype(np.float64))
    np.add.at(R, (rows, i1), l1.astype(np.float64))
    return torch.from_numpy(R)


def prompt_mix(logits, param, H, W, dout=None, absolute=False, dtype=torch.float64, fused=False):
    """logits (B, L), param (1, L, D, S, S), dout (B, D, H, W) -> y (B, D, H, W), dlogits (B, L), dparam (1, L, D, S, S);
    ``fused``: the source coordinates of lerp_taps(fused=True)"""
    B, L = logits.shape
    _, _, D, S, _ = param.shape
    My, Mx = lerp_matrix(S, H, fused), lerp_matrix(S, W, fused)
    fy, fx = int((My != 0).sum(0).max()), int((Mx != 0).sum(0).max())    # the largest footprint of a source row / column
    n = {"y": 5 * L + 4, "dparam": B * fy * fx + L, "dlogits": fy * fx + D * S * S + 2 * L}
    Ry, Rx = My.to(dtype), Mx.to(dtype)

    def resize(w, p):
        return torch.einsum("hs,bdst,wt->bdhw", Ry, torch.einsum("bl,ldst->bdst", w, p), Rx)

    lg = _leaf(logits, dtype)
    pp = _leaf(param[0], dtype, absolute)
    if not absolute:
        y = resize(softmax(lg, 1), pp)
        outs = {"y": y.detach()}
        if dout is not None:
            y.backward(dout.detach().to(dtype))
            outs.update(dlogits=lg.grad, dparam=pp.grad[None])
        return outs, n
    w = softmax(lg.detach(), 1).requires_grad_(True)     # the signed softmax weights, a leaf: w.grad[b, l] = <|dP[b]|, |param[l]|>
    y = resize(w, pp)
    outs = {"y": y.detach()}
    if dout is not None:
        y.backward(dout.detach().to(dtype).abs())
        wd = w.detach()
        outs.update(dlogits=wd * (w.grad + (wd * w.grad).sum(1, keepdim=True)), dparam=pp.grad[None])
    return outs, n


# ---- mean over the pixels + linear ---------------------------------------------------------------------------------------------
def meanpool_fc(x, fw, fb, g=None, absolute=False, dtype=torch.float64):
    """x (B, C, H, W), fw (NC, C), fb (NC,) or None, g (B, NC) -> logits, dx, dfw[, dfb]"""
    B, C, H, W = x.shape
    NC, P = fw.shape[0], H * W
    n = {"logits": P + C + 1, "dx": NC + 1, "dfw": B + P, "dfb": B}
    xr, wr = _leaf(x, dtype, absolute), _leaf(fw, dtype, absolute)
    br = None if fb is None else _leaf(fb, dtype, absolute)
    logits = F.linear(xr.mean(dim=(2, 3)), wr, br)
    outs = {"logits": logits.detach()}
    if g is not None:
        g = g.detach().to(dtype)
        logits.backward(g.abs() if absolute else g)
        outs.update(dx=xr.grad, dfw=wr.grad)
        if br is not None:
            outs["dfb"] = br.grad
    return outs, n


# ---- conv1x1 -> max-pool 2x2 -> ReLU -------------------------------------------------------------------------------------------
def windows(z):
    """the four elements of every 2 x 2 window in scan order: (0, 0), (0, 1), (1, 0), (1, 1)"""
    return [z[..., 0::2, 0::2], z[..., 0::2, 1::2], z[..., 1::2, 0::2], z[..., 1::2, 1::2]]


def route(vs):
    """torch's MaxPool2d followed by ReLU: the FIRST maximum of the window in scan order takes the gradient, and only if it is > 0.
    -> (index 0..3 of that element, mask)"""
    m, idx = vs[0], torch.zeros(vs[0].shape, dtype=torch.int64)
    for k in (1, 2, 3):
        up = vs[k] > m
        m = torch.where(up, vs[k], m)
        idx = torch.where(up, torch.full_like(idx, k), idx)
    return idx, m > 0


def _routed(vs, idx, pos):
    y = torch.zeros_like(vs[0])
    for k in range(4):
        y = y + torch.where((idx == k) & pos, vs[k], torch.zeros_like(vs[k]))
    return y


def ambiguous_windows(z, rel=1e-5, exact_ties_count=True):
    """windows whose routing a last-bit difference of z could change: the two largest values within rel * max|z| of each other, or the
    maximum within rel * max|z| of 0.  ``exact_ties_count=False`` leaves exact ties and exact zeros out (inputs that hold them on
    purpose: there the routing is the property under test)."""
    top = torch.stack(windows(z.detach())).topk(2, dim=0).values
    thr = rel * float(z.abs().max())
    gap, m = top[0] - top[1], top[0].abs()
    if exact_ties_count:
        return (gap <= thr) | (m <= thr)
    return ((gap <= thr) & (gap > 0)) | ((m <= thr) & (m > 0))


def conv1x1_pool_relu(x, w, dy=None, absolute=False, dtype=torch.float64):
    """x (B, Cin, H, W), w (Cout, Cin, 1, 1), dy (B, Cout, H/2, W/2) -> y, dx, dw and the signed conv output z.  The forward magnitude
    sum of y is the largest of its window: the maximum may be any element that a rounding makes the largest."""
    B, Cin, H, W = x.shape
    n = {"y": Cin, "dx": w.shape[0], "dw": B * (H // 2) * (W // 2)}
    xr, wr = _leaf(x, dtype), _leaf(w, dtype)
    z = F.conv2d(xr, wr)
    idx, pos = route(windows(z.detach()))
    if not absolute:
        y = _routed(windows(z), idx, pos)
        outs = {"y": y.detach(), "z": z.detach()}
        if dy is not None:
            y.backward(dy.detach().to(dtype))
            outs.update(dx=xr.grad, dw=wr.grad)
        return outs, n
    xa, wa = _leaf(x, dtype, True), _leaf(w, dtype, True)
    za = F.conv2d(xa, wa)
    outs = {"y": F.max_pool2d(za.detach(), 2, 2)}
    if dy is not None:
        _routed(windows(za), idx, pos).backward(dy.detach().to(dtype).abs())
        outs.update(dx=xa.grad, dw=wa.grad)
    return outs, n


# ---- mixing --------------------------------------------------------------------------------------------------------------------
def mix(prev, feat, mw, idx, dout=None, absolute=False, dtype=torch.float64):
    """prev (or None), feat, dout of one shape, mw (n,) -> y, dfeat, dmix[, dprev]"""
    n = {"y": 2, "dfeat": 1, "dprev": 1, "dmix": feat.numel() + mw.numel() + 2}
    if not absolute:
        fr, mr = _leaf(feat, dtype), _leaf(mw, dtype)
        pr = None if prev is None else _leaf(prev, dtype)
        y = softmax(mr, 0)[idx] * fr
        if pr is not None:
            y = pr + y
        outs = {"y": y.detach()}
        if dout is not None:
            y.backward(dout.detach().to(dtype))
            outs.update(dfeat=fr.grad, dmix=mr.grad)
            if pr is not None:
                outs["dprev"] = pr.grad
        return outs, n
    s = softmax(mw.detach().to(dtype), 0)
    fa = feat.detach().to(dtype).abs()
    y = s[idx] * fa
    if prev is not None:
        y = y + prev.detach().to(dtype).abs()
    outs = {"y": y}
    if dout is not None:
        ga = dout.detach().to(dtype).abs()
        onehot = torch.zeros_like(s)
        onehot[idx] = 1
        outs.update(dfeat=s[idx] * ga, dmix=(ga * fa).sum() * s[idx] * (onehot + s))
        if prev is not None:
            outs["dprev"] = ga
    return outs, n


# ---- image embedding -----------------------------------------------------------------------------------------------------------
def layernorm_cf(z, w, b, eps=1e-6):
    """channels-first LayerNorm: over dim 1 of (B, C, H, W), biased variance"""
    u = z.mean(1, keepdim=True)
    s = (z - u).pow(2).mean(1, keepdim=True)
    return w[:, None, None] * ((z - u) / torch.sqrt(s + eps)) + b[:, None, None]


def conv_embed_ln(x, w, b, lnw, lnb, dy=None, stride=2, pad=3, eps=1e-6, absolute=False, dtype=torch.float64):
    """x (B, Cin, H, W), w (C, Cin, k, k), b, lnw, lnb (C,) -> y, dx, dw, db, dlnw, dlnb"""
    B, Cin, H, W = x.shape
    C, _, ks, _ = w.shape
    K = Cin * ks * ks + 1
    taps = (-(-ks // stride)) ** 2
    xr, wr, br, lwr, lbr = (_leaf(t, dtype) for t in (x, w, b, lnw, lnb))
    z = F.conv2d(xr, wr, br, stride=stride, padding=pad)
    M = B * z.shape[2] * z.shape[3]
    n = {"y": K + 2 * C + 2, "dx": C * taps + K + 4 * C, "dw": M + K + 4 * C, "db": M + K + 4 * C, "dlnw": M + K + 2 * C, "dlnb": M}
    if not absolute:
        y = layernorm_cf(z, lwr, lbr, eps)
        outs = {"y": y.detach()}
        if dy is not None:
            y.backward(dy.detach().to(dtype))
            outs.update(dx=xr.grad, dw=wr.grad, db=br.grad, dlnw=lwr.grad, dlnb=lbr.grad)
        return outs, n
    z = z.detach()
    rstd = 1.0 / torch.sqrt((z - z.mean(1, keepdim=True)).pow(2).mean(1, keepdim=True) + eps)     # of the signed run
    xa, wa, ba = (_leaf(t, dtype, True) for t in (x, w, b))
    za = F.conv2d(xa, wa, ba, stride=stride, padding=pad)
    zd = za.detach()
    xh = (zd + zd.mean(1, keepdim=True)) * rstd                     # |z - mean| / sigma without the cancellation
    lwa = lnw.detach().to(dtype).abs()[:, None, None]
    outs = {"y": lwa * xh + lnb.detach().to(dtype).abs()[:, None, None]}
    if dy is not None:
        g = dy.detach().to(dtype).abs()
        gp = g * lwa
        dz = rstd * (gp + gp.mean(1, keepdim=True) + xh * (gp * xh).mean(1, keepdim=True))
        (za * dz).sum().backward()
        outs.update(dx=xa.grad, dw=wa.grad, db=ba.grad, dlnw=(g * xh).sum(dim=(0, 2, 3)), dlnb=g.sum(dim=(0, 2, 3)))
    return outs, n
