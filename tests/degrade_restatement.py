"""A kernel-blind restatement of the demosaic and line-mask degradations (include/dcpt_hip.h dcpt_demosaic_fwd, dcpt_inpaint_lines_fwd) in
numpy int64 and Python integers, one pixel at a time, written from the header's statement of the arithmetic and not from the kernel: the
5 x 5 Malvar tables in units of 1/16 over ``np.pad(..., "reflect")``, the 3 x 3 bilinear tables in units of 1/4 over the three sparse
planes padded with ``"wrap"``, the rounding of S / unit to the 8-bit grid by integer division (half to even), and the distance rule of the
strokes.  Integer inputs give exact integer sums; float64 inputs give the float64 form of the same sums."""
import numpy as np

# units of 1/16
KGRB = np.array([[0, 0, -2, 0, 0], [0, 0, 4, 0, 0], [-2, 4, 8, 4, -2], [0, 0, 4, 0, 0], [0, 0, -2, 0, 0]], dtype=np.int64)
KRBG0 = np.array([[0, 0, 1, 0, 0], [0, -2, 0, -2, 0], [-2, 8, 10, 8, -2], [0, -2, 0, -2, 0], [0, 0, 1, 0, 0]], dtype=np.int64)
KRBBR = np.array([[0, 0, -3, 0, 0], [0, 4, 0, 4, 0], [-3, 0, 12, 0, -3], [0, 4, 0, 4, 0], [0, 0, -3, 0, 0]], dtype=np.int64)
IDENT = np.zeros((5, 5), dtype=np.int64)
IDENT[2, 2] = 16
# units of 1/4
K_RB = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], dtype=np.int64)
K_G = np.array([[0, 1, 0], [1, 4, 1], [0, 1, 0]], dtype=np.int64)


def colour(r, c):
    """0 R, 1 G, 2 B of the RGGB site (r, c)"""
    return 1 if (r + c) % 2 else (0 if r % 2 == 0 else 2)


def to_u8(x):
    """rint(clamp(x, 0, 1) * 255) with the product in fp32, as int64"""
    x = np.asarray(x, dtype=np.float32)
    return np.rint(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.int64)


def cfa_of(v):
    """(B, C, H, W) -> the (B, H, W) CFA plane: channel 0 when C == 1, else the channel of each site's colour"""
    v = np.asarray(v)
    b, c, h, w = v.shape
    if c == 1:
        return v[:, 0].copy()
    out = np.empty((b, h, w), dtype=v.dtype)
    for r in range(h):
        for q in range(w):
            out[:, r, q] = v[:, colour(r, q), r, q]
    return out


def _malvar_table(ch, r, c):
    site = colour(r, c)
    if site == ch:
        return IDENT
    if ch == 1:
        return KGRB
    if site == 1:   # R or B at a G site: the row kernel where the row holds that colour
        row_has_ch = (r % 2 == 0) if ch == 0 else (r % 2 == 1)
        return KRBG0 if row_has_ch else KRBG0.T
    return KRBBR


def malvar_sums(cfa):
    """(B, H, W) -> (B, 3, H, W) sums in units of 1/16 (the dtype of ``cfa``: int64 stays exact)"""
    cfa = np.asarray(cfa)
    b, h, w = cfa.shape
    pad = np.pad(cfa, ((0, 0), (2, 2), (2, 2)), mode="reflect")
    out = np.zeros((b, 3, h, w), dtype=cfa.dtype)
    for r in range(h):
        for c in range(w):
            win = pad[:, r:r + 5, c:c + 5]
            for ch in range(3):
                out[:, ch, r, c] = (win * _malvar_table(ch, r, c)).sum(axis=(1, 2))
    return out


def bilinear_sums(cfa):
    """(B, H, W) -> (B, 3, H, W) sums in units of 1/4: the sparse colour planes, circular padding, 3 x 3"""
    cfa = np.asarray(cfa)
    b, h, w = cfa.shape
    sparse = np.zeros((b, 3, h, w), dtype=cfa.dtype)
    for r in range(h):
        for c in range(w):
            sparse[:, colour(r, c), r, c] = cfa[:, r, c]
    pad = np.pad(sparse, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="wrap")
    out = np.zeros((b, 3, h, w), dtype=cfa.dtype)
    for r in range(h):
        for c in range(w):
            for ch in range(3):
                out[:, ch, r, c] = (pad[:, ch, r:r + 3, c:c + 3] * (K_G if ch == 1 else K_RB)).sum(axis=(1, 2))
    return out


def round_to_grid(s, unit):
    """rint(clamp(S / unit, 0, 255)), half to even, in integers"""
    s = np.asarray(s, dtype=np.int64)
    q, r = np.divmod(s, unit)
    q = q + ((2 * r > unit) | ((2 * r == unit) & (q % 2 == 1)))
    return np.clip(q, 0, 255)


def sums(cfa, method):
    return (malvar_sums(cfa), 16) if method == "malvar" else (bilinear_sums(cfa), 4)


def demosaic_u8(x, method="malvar"):
    """the uint8_io result as float32 (B, 3, H, W), with the sums S and the unit"""
    s, unit = sums(cfa_of(to_u8(x)), method)
    return round_to_grid(s, unit).astype(np.float32) / np.float32(255), s, unit


def demosaic_f64(x, method="malvar"):
    """sum w x in float64"""
    s, unit = sums(cfa_of(np.asarray(x, dtype=np.float64)), method)
    return s / unit


def line_mask(lines, meta, h, w):
    """boolean (H, W): within thick / 2 of one of the first n_lines segments, in Python integers"""
    n, thick = int(meta[0]), int(meta[1])
    mask = np.zeros((h, w), dtype=bool)
    t2 = thick * thick
    for x1, y1, x2, y2 in [[int(v) for v in row] for row in np.asarray(lines)[:n]]:
        dx, dy = x2 - x1, y2 - y1
        big_l = dx * dx + dy * dy
        for py in range(h):
            for px in range(w):
                qx, qy = px - x1, py - y1
                a = qx * dx + qy * dy
                if a <= 0:
                    hit = 4 * (qx * qx + qy * qy) <= t2
                elif a >= big_l:
                    hit = 4 * ((qx - dx) ** 2 + (qy - dy) ** 2) <= t2
                else:
                    hit = 4 * (qx * dy - qy * dx) ** 2 <= t2 * big_l
                if hit:
                    mask[py, px] = True
    return mask


def inpaint(x, lines, meta):
    """(B, C, H, W) float32 -> the degraded batch and the (B, H, W) masks"""
    x = np.asarray(x, dtype=np.float32)
    b, _, h, w = x.shape
    y = np.clip(x, np.float32(0), np.float32(1))
    masks = np.zeros((b, h, w), dtype=bool)
    for i in range(b):
        masks[i] = line_mask(np.asarray(lines)[i], np.asarray(meta)[i], h, w)
        y[i][:, masks[i]] = np.float32(1 if int(np.asarray(meta)[i][2]) else 0)
    return y, masks
