"""The two halves of a SwinIR block (the DCPT variant: no relative-position bias, no shift mask) restated in plain torch, stage by stage.

    attention half   y = x + proj(WMSA_shift(qkv(LN1(x))))        attn_half
    MLP half         y = x + fc2(gelu(fc1(LN2(x))))               mlp_half

Both run in the dtype of their inputs (float64: the truth; float32: the yardstick) on the CPU and return every stage in the layout the
HIP kernels store (dcpt_amd.functional._SwinAttnFn / _SwinMlpFn): token rows are the NHWC pixel rows, M = B H W of them, in pixel order --
never in window order.  ``x`` and ``y`` are (B, C, H, W); ``P`` is keyed like a SwinTransformerBlock's state dict.

The cyclic shift (torch.roll by -shift), the window partition, the window reverse and the inverse roll are ONE explicit index map
(``window_rows``): token t = i ws + j of window (wy, wx) of image b is pixel ((wy ws + i + shift) mod H, (wx ws + j + shift) mod W);
windows are gathered through it and scattered back through it.

``mut`` names deliberate mistakes (MUTATIONS); tests/test_swin_restatement_cpu.py asserts which case of the GPU test tells which of them
from the right thing.  With ``mut`` empty nothing of that is in the way.

``attn_grads`` / ``mlp_grads``: autograd of the above (dx and the six parameter gradients) plus, for every gradient that is a sum over the
tokens -- LayerNorm weight and bias, the three biases -- the sum of the MAGNITUDES of its terms ("mag.g.<name>"): an fp32 sum of terms of
both signs is good to an ulp of what it added up, not of what is left."""
import math

import torch

LN_EPS = 1e-5
MUTATIONS = ("roll_sign", "no_inverse_roll", "shift_y_only", "shift_x_only", "clamp", "ij_transposed", "grid_transposed", "qkv_heads_first",
             "scale_dp", "pad_keys", "v_pad_leak", "lse_no_max", "lse_unscaled", "eps_1e6", "unbiased_var", "tanh_gelu", "gelu_no_xpdf")


def padded(n):
    """the kernel's padded extent of n tokens / n head channels"""
    return 32 if n <= 32 else 64


def window_rows(B, H, W, ws, sy, sx, wrap=True, grid_t=False, ij_t=False):
    """(B nwy nwx, ws ws) int64: the NHWC pixel row of every token of every window, windows in (b, wy, wx) order"""
    nwy, nwx = H // ws, W // ws
    r = torch.arange(nwy * nwx)
    wy, wx = (r // nwy, r % nwy) if grid_t else (r // nwx, r % nwx)
    t = torch.arange(ws * ws)
    i, j = (t % ws, t // ws) if ij_t else (t // ws, t % ws)
    py = wy[:, None] * ws + i[None, :] + sy
    px = wx[:, None] * ws + j[None, :] + sx
    py, px = (py % H, px % W) if wrap else (py.clamp(max=H - 1), px.clamp(max=W - 1))
    rows = py * W + px
    return (torch.arange(B)[:, None, None] * (H * W) + rows[None]).reshape(B * nwy * nwx, ws * ws)


def _maps(B, H, W, ws, shift, mut):
    """(the map the windows are gathered through, the map they are scattered back through): the same one unless ``mut`` says otherwise"""
    sy = sx = -shift if "roll_sign" in mut else shift
    if "shift_y_only" in mut:
        sx = 0
    if "shift_x_only" in mut:
        sy = 0
    kw = dict(wrap="clamp" not in mut, grid_t="grid_transposed" in mut)
    src = window_rows(B, H, W, ws, sy, sx, **kw)
    if "no_inverse_roll" in mut:
        return src, window_rows(B, H, W, ws, 0, 0, **kw)
    if "ij_transposed" in mut:
        return src, window_rows(B, H, W, ws, sy, sx, ij_t=True, **kw)
    if not mut:
        assert torch.equal(src.flatten().sort().values, torch.arange(B * H * W)), "the window map is not a permutation of the pixels"
    return src, src


def _scatter(win, idx, M):
    """rows of ``win`` (nw, N, cols) back to their pixels; a pixel no token maps to stays 0 (none, with the right map)"""
    return torch.zeros(M, win.shape[-1], dtype=win.dtype).index_add(0, idx.reshape(-1), win.reshape(-1, win.shape[-1]))


def layer_norm(rows, w, b, mut=()):
    """-> mu (M,), rstd (M,), LN(rows) (M, C): biased variance, eps 1e-5"""
    C = rows.shape[1]
    mu = rows.mean(1)
    d = rows - mu[:, None]
    var = (d * d).sum(1) / (C - 1 if "unbiased_var" in mut else C)
    rstd = 1.0 / torch.sqrt(var + (1e-6 if "eps_1e6" in mut else LN_EPS))
    return mu, rstd, d * rstd[:, None] * w + b


def _rows(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C)


def _map(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def attn_half(x, P, heads, ws, shift, mut=()):
    """-> {mu, rstd (M,); xn (M, C); qkv (M, 3C), column s C + h hd + d; lse (M, heads), of the SCALED scores; att (M, C); y (B, C, H, W)}"""
    B, C, H, W = x.shape
    hd, N, M = C // heads, ws * ws, B * H * W
    rows = _rows(x)
    mu, rstd, xn = layer_norm(rows, P["norm1.weight"], P["norm1.bias"], mut)
    qkv = xn @ P["attn.qkv.weight"].t() + P["attn.qkv.bias"]
    src, dst = _maps(B, H, W, ws, shift, mut)
    nw = src.shape[0]
    win = qkv[src]                                                        # (nw, N, 3C)
    if "qkv_heads_first" in mut:
        q, k, v = win.reshape(nw, N, heads, 3, hd).permute(3, 0, 2, 1, 4)
    else:
        q, k, v = win.reshape(nw, N, 3, heads, hd).permute(2, 0, 3, 1, 4)   # each (nw, heads, N, hd)
    scale = (padded(hd) if "scale_dp" in mut else hd) ** -0.5
    s = (q * scale) @ k.transpose(-1, -2)                                 # q is scaled before the product, as the reference does
    if "pad_keys" in mut:
        s = torch.cat([s, s.new_zeros(nw, heads, N, padded(N) - N)], -1)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    den = e.sum(-1, keepdim=True)
    p = (e / den)[..., :N]
    lse = mx + torch.log(den)
    if "lse_no_max" in mut:      # in fp32, where it overflows (float64 would carry e^200)
        lse = torch.log(torch.exp(s.float()).sum(-1, keepdim=True)).to(s.dtype)
    if "lse_unscaled" in mut:
        lse = torch.logsumexp(q @ k.transpose(-1, -2), -1, keepdim=True)
    o = (p @ v).permute(0, 2, 1, 3)                                       # (nw, N, heads, hd)
    if "v_pad_leak" in mut:      # the zero pad columns hd .. DP of head h's tile written over the first columns of head h + 1
        lead = min(padded(hd) - hd, hd)
        keep = torch.ones(heads, hd, dtype=o.dtype)
        keep[1:, :lead] = 0
        o = o * keep
    att = _scatter(o.reshape(nw, N, C), dst, M)
    lse = _scatter(lse.squeeze(-1).permute(0, 2, 1), dst, M)
    y = rows + att @ P["attn.proj.weight"].t() + P["attn.proj.bias"]
    return dict(mu=mu, rstd=rstd, xn=xn, qkv=qkv, lse=lse, att=att, y=_map(y, B, H, W))


class _Gelu(torch.autograd.Function):
    """erf GELU with its derivative written out: cdf(h) + h pdf(h)"""

    @staticmethod
    def forward(ctx, h, no_xpdf):
        ctx.save_for_backward(h)
        ctx.no_xpdf = no_xpdf
        return 0.5 * h * (1.0 + torch.erf(h * math.sqrt(0.5)))

    @staticmethod
    def backward(ctx, g):
        h, = ctx.saved_tensors
        cdf = 0.5 * (1.0 + torch.erf(h * math.sqrt(0.5)))
        pdf = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
        return g * (cdf if ctx.no_xpdf else cdf + h * pdf), None


def gelu(h, mut=()):
    if "tanh_gelu" in mut:
        return 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))
    return _Gelu.apply(h, "gelu_no_xpdf" in mut)


def mlp_half(x, P, mut=()):
    """-> {mu, rstd (M,); xn (M, C); h (M, hidden): fc1's output BEFORE the GELU; y (B, C, H, W)}"""
    B, C, H, W = x.shape
    rows = _rows(x)
    mu, rstd, xn = layer_norm(rows, P["norm2.weight"], P["norm2.bias"], mut)
    h = xn @ P["mlp.fc1.weight"].t() + P["mlp.fc1.bias"]
    y = rows + gelu(h, mut) @ P["mlp.fc2.weight"].t() + P["mlp.fc2.bias"]
    return dict(mu=mu, rstd=rstd, xn=xn, h=h, y=_map(y, B, H, W))


def _grads(half, norm, pre_bias, out_bias, x, dy, P, dtype):
    """stages + dx + "g.<key>" + "mag.g.<key>" of one half; ``pre_bias``: (bias key, stage whose rows its gradient column-sums)"""
    P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in P.items()}
    x = x.detach().clone().to(dtype).requires_grad_(True)
    st = half(x, P)
    st["xn"].retain_grad()
    st[pre_bias[1]].retain_grad()
    st["y"].backward(dy.to(dtype))
    out = {k: v.detach() for k, v in st.items()}
    out["dx"] = x.grad
    out.update({"g." + k: p.grad for k, p in P.items()})
    dxn = st["xn"].grad
    xhat = (_rows(x.detach()) - out["mu"][:, None]) * out["rstd"][:, None]
    out["mag.g." + norm + ".weight"] = (dxn * xhat).abs().sum(0)
    out["mag.g." + norm + ".bias"] = dxn.abs().sum(0)
    out["mag.g." + pre_bias[0]] = st[pre_bias[1]].grad.abs().sum(0)
    out["mag.g." + out_bias] = _rows(dy.to(dtype)).abs().sum(0)
    for k in (norm + ".weight", norm + ".bias", pre_bias[0], out_bias):     # the sums themselves, from the same terms
        assert torch.allclose({norm + ".weight": (dxn * xhat).sum(0), norm + ".bias": dxn.sum(0), pre_bias[0]: st[pre_bias[1]].grad.sum(0),
                               out_bias: _rows(dy.to(dtype)).sum(0)}[k], out["g." + k], rtol=1e-4, atol=1e-5 * float(out["mag.g." + k].max()))
    return out


def attn_grads(x, dy, P, heads, ws, shift, dtype, mut=()):
    return _grads(lambda x_, P_: attn_half(x_, P_, heads, ws, shift, mut), "norm1", ("attn.qkv.bias", "qkv"), "attn.proj.bias", x, dy, P, dtype)


def mlp_grads(x, dy, P, dtype, mut=()):
    return _grads(lambda x_, P_: mlp_half(x_, P_, mut), "norm2", ("mlp.fc1.bias", "h"), "mlp.fc2.bias", x, dy, P, dtype)
