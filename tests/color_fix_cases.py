"""The yardstick of the colour-fix tests: StableSR's ``wavelet_reconstruction`` and ``adaptive_instance_normalization`` restated in
PyTorch in their LITERAL form (two wavelet decompositions with ``F.conv2d`` on ``F.pad(mode='replicate')``; ``var`` unbiased + 1e-5),
evaluated in float64 unless a dtype is given, plus the one-chain separable form the kernels compute, which
``tests/test_color_fix_cpu.py`` checks against the literal form.  Test infrastructure only: product code never imports it."""
import torch
import torch.nn.functional as F

SIZES = [(5, 7), (20, 37), (33, 64), (256, 256), (300, 500)]      # 5x7: smaller than radii 8 and 16; 20x37, 33x64 straddle r = 16
RADII = (1, 2, 4, 8, 16)


def wavelet_blur(image, radius):
    """[N,3,H,W]: the 3x3 kernel [1,2,1]^T [1,2,1] / 16 with dilation ``radius`` per channel on a replicate-padded image."""
    k = torch.tensor([[0.0625, 0.125, 0.0625], [0.125, 0.25, 0.125], [0.0625, 0.125, 0.0625]], dtype=image.dtype, device=image.device)
    k = k[None, None].repeat(3, 1, 1, 1)
    image = F.pad(image, (radius, radius, radius, radius), mode="replicate")
    return F.conv2d(image, k, groups=3, dilation=radius)


def wavelet_decomposition(image, levels=5):
    high = torch.zeros_like(image)
    low = image
    for i in range(levels):
        low = wavelet_blur(image, 2 ** i)
        high = high + (image - low)
        image = low
    return high, low


def wavelet_literal(content, style, dtype=torch.float64):
    """high5(content) + low5(style), before the final clamp.  [3,H,W] or [N,3,H,W]."""
    c, s = content.to(dtype), style.to(dtype)
    squeeze = c.dim() == 3
    if squeeze:
        c, s = c[None], s[None]
    out = wavelet_decomposition(c)[0] + wavelet_decomposition(s)[1]
    return out[0] if squeeze else out


def adain_literal(content, style, dtype=torch.float64, eps=1e-5):
    """(content - mean_c) / std_c * std_s + mean_s per channel, std = sqrt(unbiased variance + eps); before the final clamp."""
    c, s = content.to(dtype), style.to(dtype)
    squeeze = c.dim() == 3
    if squeeze:
        c, s = c[None], s[None]
    n, ch = c.shape[:2]

    def mean_std(t):
        var = t.reshape(n, ch, -1).var(dim=2) + eps
        return t.reshape(n, ch, -1).mean(dim=2).view(n, ch, 1, 1), var.sqrt().view(n, ch, 1, 1)
    mc, sc = mean_std(c)
    ms, ss = mean_std(s)
    out = (c - mc.expand_as(c)) / sc.expand_as(c) * ss.expand_as(c) + ms.expand_as(c)
    return out[0] if squeeze else out


def literal(mode, content, style, dtype=torch.float64):
    return {"wavelet": wavelet_literal, "adain": adain_literal}[mode](content, style, dtype)


def blur_separable(x, radius):
    """One level as the kernels compute it: 0.25 x[clamp(i-r)] + 0.5 x[i] + 0.25 x[clamp(i+r)] along x, then along y."""
    h, w = x.shape[-2:]
    ix = torch.arange(w)
    x = 0.25 * x[..., (ix - radius).clamp(0, w - 1)] + 0.5 * x + 0.25 * x[..., (ix + radius).clamp(0, w - 1)]
    iy = torch.arange(h)
    return 0.25 * x[..., (iy - radius).clamp(0, h - 1), :] + 0.5 * x + 0.25 * x[..., (iy + radius).clamp(0, h - 1), :]


def wavelet_one_chain(content, style, dtype=torch.float64):
    """content + B16(B8(B4(B2(B1(style - content))))): equal to ``wavelet_literal`` because the clamped blur is linear."""
    c, s = content.to(dtype), style.to(dtype)
    d = s - c
    for r in RADII:
        d = blur_separable(d, r)
    return c + d


def pair(h, w, seed, mode):
    """A seeded (content, condition) pair [3,h,w] fp32 in [0,1]; for adain the condition is 0.25 + 0.5 rand, so that
    std_s / std_c = 0.5 (inside [0.5, 2], the range the adain tolerance is derived for)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(3, h, w, generator=g)
    s = torch.rand(3, h, w, generator=g)
    if mode == "adain":
        s = 0.25 + 0.5 * s
    return c, s
