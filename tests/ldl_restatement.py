"""A kernel-blind restatement, in torch float64 on the CPU, of the LDL artifact-weight map -- the yardstick of tests/test_ldl_cpu.py and
tests/test_gpu_ldl.py.  Not a test.  It is written from the formulas and knows nothing of tiles, planes or workspaces:

    r = |gt - out|
    u = unbiased std of r over the 7 x 7 window around each pixel, r reflect-padded by 3      (pad, unfold, torch.std)
    m = mean(u), s = unbiased std(u) over all elements
    w = (tanh((u - m) / s) + 1) / 2

which is the one path of the reference's get_refined_artifact_map (basicsr/losses/loss_util.py:100-165) that its SRModel reaches: std=True,
ksize 7, no img_ema.  ``artifact_map`` takes float64 tensors (fp32 values widened by the caller: the difference is then exact, where the
reference rounds it to fp32); its gradient comes from torch autograd.

``weight_grad_closed_form`` is a second, independent yardstick: the gradient of sum(Gw * w) with respect to ``out`` written out by hand,

    t = tanh z, z = (u - m) / s
    Gz = Gw (1 - t^2) / 2
    Gu = (Gz - mean(Gz) - z sum(Gz z) / (N - 1)) / s
    Gv = Gu / (2 u), 0 where u == 0                       (torch's std backward masks u == 0 the same way)
    Gr = (2 / 48) (r T(Gv) - T(Gv mu)),  mu the window mean of r
    Gout = Gr sign(out - gt)

with T the transpose of "reflect-pad by 3, then 7 x 7 box": the 7 x 7 box sum of the plane over the padded domain (H + 6) x (W + 6), the
plane counting as zero outside itself, then folded back per axis (padded index q < 0 to -q, q >= W to 2 (W - 1) - q)."""
import torch
import torch.nn.functional as F

K, PAD = 7, 3


def local_std(r):
    """unbiased std over the 7 x 7 window around each pixel of the reflect-padded r (B, C, H, W)"""
    p = F.pad(r, [PAD, PAD, PAD, PAD], mode="reflect")
    return torch.std(p.unfold(2, K, 1).unfold(3, K, 1), dim=(-1, -2), unbiased=True)


def local_mean(r):
    p = F.pad(r, [PAD, PAD, PAD, PAD], mode="reflect")
    return p.unfold(2, K, 1).unfold(3, K, 1).mean(dim=(-1, -2))


def artifact_map(gt, out):
    u = local_std((gt - out).abs())
    return (((u - u.mean()) / u.std()).tanh() + 1) / 2


def ldl_term(gt, out, elementwise_loss):
    """``(w * cri_ldl(out, gt)).mean()`` of the reference's training step (basicsr/models/sr_model.py:145-153); the weights are not detached"""
    return (artifact_map(gt, out) * elementwise_loss).mean()


def _fold(x, dim):
    """add the 3 leading and the 3 trailing entries of the padded axis back onto the entries they were reflected from"""
    n = x.shape[dim] - 2 * PAD
    core = x.narrow(dim, PAD, n).clone()
    for q in range(1, PAD + 1):
        core.narrow(dim, q, 1).add_(x.narrow(dim, PAD - q, 1))                 # padded index -q -> q
        core.narrow(dim, n - 1 - q, 1).add_(x.narrow(dim, PAD + n - 1 + q, 1))  # padded index n - 1 + q -> n - 1 - q
    return core


def box_transpose(g):
    """T(g): 7 x 7 box sum over the padded domain of the zero-extended plane, folded back per axis"""
    B, C, H, W = g.shape
    z = F.pad(g, [2 * PAD] * 4)   # zero outside the plane, far enough for a box around every padded position
    box = F.avg_pool2d(z, K, stride=1) * (K * K)   # (H + 6) x (W + 6)
    return _fold(_fold(box, 3), 2)


def weight_grad_closed_form(gt, out, gw):
    r = (gt - out).abs()
    u, mu = local_std(r), local_mean(r)
    n = u.numel()
    z = (u - u.mean()) / u.std()
    gz = gw * (1 - z.tanh() ** 2) / 2
    gu = (gz - gz.mean() - z * (gz * z).sum() / (n - 1)) / u.std()
    gv = torch.where(u == 0, torch.zeros_like(u), gu / (2 * u))
    gr = (2.0 / 48.0) * (r * box_transpose(gv) - box_transpose(gv * mu))
    return gr * torch.sign(out - gt)
