"""A kernel-blind restatement, in torch float64 on the CPU, of what the SSIM losses compute -- the yardstick of tests/test_ssim_loss_cpu.py
and tests/test_gpu_ssim_loss.py.  Not a test.  It follows the reference line by line and knows nothing of tiles, planes or chunks:

* ``gauss``: cv2.getGaussianKernel(11, 1.5) from its formula (the reference needs cv2, which is not installed, so nothing here is a golden
  file of the reference; the values are compared with basicsr.metrics._gauss_kernel in the CPU test);
* ``ssim_map`` / ``ssim_pt``: ``_ssim_pth`` (basicsr/metrics/psnr_ssim.py:515-559) with grouped ``F.conv2d`` and ``calculate_ssim_pt``
  (:436-480): crop, optional luma, ``.to(float64)``;
* ``luma``: ``rgb2ycbcr_pt(y_only=True)`` (basicsr/utils/color_util.py:222-254).  There it is an fp32 matmul, whose order of summation is
  not specified; here it is fp32 element-wise ops in the documented order Y = (((r 65.481f + g 128.553f) + b 24.966f) + 16.0f) / 255.0f,
  then ``.double()``.  Its GRADIENT is that of the same expression evaluated in float64 with the fp32 coefficients (dY times
  (65.481f, 128.553f, 24.966f) / 255): autograd through the fp32 ops would round the gradient three more times, and a yardstick should not
  carry roundings of its own.  (Value from one expression, gradient from the other: ``v32.detach() + (v64 - v64.detach())``.)
* ``huber_loss`` / ``weight_reduce_loss`` / ``mse``: basic_loss.py:30-36, loss_util.py:27-56.  The element-wise values are fp32 ops on the
  fp32 inputs, as in the reference; they are ADDED UP in float64: the reference's fp32 ``.mean()`` is defined only up to the summation
  order of the device it runs on (~1e-7 relative), and the float64 sum of the same fp32 terms is the value every such order approximates;
* ``ssim_loss`` / ``ssim_mse_loss``: the two classes' expressions (basic_loss.py:175-190, :216-232), including the ``[0]`` of SSIMLoss.

Gradients come from torch autograd.  ``pred`` may be an fp32 leaf (the gradient is then rounded once to fp32, where ``.to(float64)`` is
differentiated) or a float64 leaf holding fp32 values (the gradient stays float64)."""
import numpy as np
import torch
import torch.nn.functional as F

YCOEF = (65.481, 128.553, 24.966)


def gauss():
    x = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(x ** 2) / (2 * 1.5 ** 2))
    return torch.from_numpy(g / g.sum())


def luma_ordered32(img32):
    """fp32, the documented order"""
    r, g, b = img32[:, 0:1], img32[:, 1:2], img32[:, 2:3]
    return (((r * YCOEF[0] + g * YCOEF[1]) + b * YCOEF[2]) + 16.0) / 255.0


def luma_matmul32(img32):
    """fp32, the reference's form: a matmul over the channel axis"""
    w = torch.tensor([[YCOEF[0]], [YCOEF[1]], [YCOEF[2]]], dtype=torch.float32)
    return (torch.matmul(img32.permute(0, 2, 3, 1), w).permute(0, 3, 1, 2) + 16.0) / 255.0


def luma(img):
    """float64 (B, 1, H, W): the value of ``luma_ordered32``, the gradient of the same expression in float64 with the fp32 coefficients"""
    v32 = luma_ordered32(img.detach().float()).double()
    c = torch.tensor(YCOEF, dtype=torch.float32).double().view(1, 3, 1, 1)
    v64 = ((img.double() * c).sum(1, keepdim=True) + 16.0) / 255.0
    return v32 + (v64 - v64.detach())


def ssim_map(x, y, image_range=1.0):
    """_ssim_pth on float64 (B, C, H, W): the (B, C, H - 10, W - 10) map"""
    c1, c2 = (0.01 * image_range) ** 2, (0.03 * image_range) ** 2
    g = gauss()
    C = x.shape[1]
    win = torch.outer(g, g).view(1, 1, 11, 11).expand(C, 1, 11, 11).to(x.dtype)
    cv = lambda t: F.conv2d(t, win, stride=1, padding=0, groups=C)  # noqa: E731
    mu1, mu2 = cv(x), cv(y)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = cv(x * x) - mu1_sq, cv(y * y) - mu2_sq, cv(x * y) - mu12
    cs = (2 * s12 + c2) / (s1 + s2 + c2)
    return ((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs


def prepared(img, img2, crop_border, test_y_channel):
    """calculate_ssim_pt up to the float64 pair"""
    assert img.shape == img2.shape
    if crop_border != 0:
        img = img[:, :, crop_border:-crop_border, crop_border:-crop_border]
        img2 = img2[:, :, crop_border:-crop_border, crop_border:-crop_border]
    if test_y_channel and img.shape[1] == 3:
        return luma(img), luma(img2)
    return img.to(torch.float64), img2.to(torch.float64)


def ssim_pt(img, img2, crop_border=0, test_y_channel=False, image_range=1.0):
    x, y = prepared(img, img2, crop_border, test_y_channel)
    return ssim_map(x, y, image_range).mean([1, 2, 3])


def ssim_grad_analytic(x, y, w, image_range=1.0):
    """the gradient of sum_{b,c} w[b][c] sum_p S with respect to x by the closed form the kernels use, in separable passes: float64
    (B, C, H, W) in, the same shape out"""
    c1, c2 = (0.01 * image_range) ** 2, (0.03 * image_range) ** 2
    g = gauss()
    B, C, H, W = x.shape

    def sep(t):   # "valid": rows then columns
        t = F.conv2d(t.reshape(B * C, 1, H, W), g.view(1, 1, 1, 11))
        return F.conv2d(t, g.view(1, 1, 11, 1)).reshape(B, C, H - 10, W - 10)

    def sep_t(t):   # transposed ("full"): columns then rows
        t = F.conv_transpose2d(t.reshape(B * C, 1, H - 10, W - 10), g.view(1, 1, 11, 1))
        return F.conv_transpose2d(t, g.view(1, 1, 1, 11)).reshape(B, C, H, W)

    mx, my = sep(x), sep(y)
    sxx, syy, sxy = sep(x * x) - mx * mx, sep(y * y) - my * my, sep(x * y) - mx * my
    A1, A2, B1, B2 = 2 * mx * my + c1, 2 * sxy + c2, mx * mx + my * my + c1, sxx + syy + c2
    S = A1 * A2 / (B1 * B2)
    w = w.view(B, C, 1, 1)
    Pa = w * (2 * my * (A2 - A1) / (B1 * B2) - S * (2 * mx / B1 - 2 * mx / B2))
    Pb = -w * S / B2
    Pc = 2 * w * A1 / (B1 * B2)
    return sep_t(Pa) + 2 * x * sep_t(Pb) + y * sep_t(Pc)


def weight_reduce_loss(loss, weight=None, reduction="mean"):
    """loss_util.py:27-56 over fp32 element-wise terms, added up in float64"""
    if weight is not None:
        assert weight.dim() == loss.dim() and weight.size(1) in (1, loss.size(1))
        loss = loss * weight
    loss = loss.double()
    if weight is None or reduction == "sum":
        return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss
    if reduction == "mean":
        wsum = weight.double().sum()
        return loss.sum() / (wsum if weight.size(1) > 1 else wsum * loss.size(1))
    return loss


def huber_loss(pred, target, weight=None, reduction="mean", delta=0.01):
    err = torch.abs(pred - target)
    q = torch.clamp(err, max=delta)   # the quadratic part; what is left of |d| is the linear part
    return weight_reduce_loss(0.5 * torch.pow(q, 2) + (err - q), weight, reduction)


def ssim_loss(pred, target, weight=None, ssim_weight=0.1, mse_weight=1.0, crop_border=0, reduction="mean", test_y_channel=False):
    """SSIMLoss.forward: the [0] picks the first image's SSIM before the mean"""
    s = ssim_pt(pred, target, crop_border, test_y_channel, 1)[0].mean()
    return ssim_weight * (1 - s) + mse_weight * huber_loss(pred, target, weight, reduction)


def ssim_mse_loss(pred, target, ssim_weight=0.1, mse_weight=1.0, crop_border=0, reduction="mean", test_y_channel=False):
    s = ssim_pt(pred, target, crop_border, test_y_channel, 1).mean()
    return ssim_weight * (1 - s) + mse_weight * weight_reduce_loss(F.mse_loss(pred, target, reduction="none"), None, reduction)
