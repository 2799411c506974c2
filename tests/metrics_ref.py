"""Restatements of the clip-comparison statistics in plain torch on the CPU (TEST INFRASTRUCTURE).  Nothing here imports
landiff_amd: the window table is built here a second time and compared with the product's in the host tests.

diff_ref: the integer statistics in int64.
ssim_ref64: SSIM by its definition in float64, with the fp32-rounded window table upcast.
ssim_ref32: the same definition in fp32 in the kernel's order -- x - 128, rows first then columns, taps added in ascending order,
every product and sum rounded on its own -- which is the yardstick of the GPU test: its distance from ssim_ref64 on a case is
what fp32 costs there, and the kernel is allowed four times the largest such distance of the case's family."""
import numpy as np
import torch

TAPS, SIGMA = 11, 1.5
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def window32() -> torch.Tensor:
    """The 11-tap Gaussian of sigma 1.5, normalised in float64, rounded to fp32 once."""
    x = np.arange(TAPS, dtype=np.float64) - (TAPS - 1) / 2
    g = np.exp(-(x * x) / (2.0 * SIGMA * SIGMA))
    return torch.from_numpy((g / g.sum()).astype(np.float32))


def diff_ref(a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [F, H, W, C] x 2, bool [F, H, W] or None -> int64 [F, C, 5]: n, sum d^2, sum |d|, max |d|, number of d != 0."""
    d = (a.long() - b.long()).abs()
    keep = torch.ones(a.shape[:3], dtype=torch.bool) if mask is None else mask
    k = keep[..., None].expand_as(d).long()
    dk = d * k
    return torch.stack([k.sum((1, 2)), (dk * dk).sum((1, 2)), dk.sum((1, 2)), dk.amax((1, 2)), (dk != 0).long().sum((1, 2))], dim=-1)


def _blur(q: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[F, H, W, C] -> [F, H-10, W-10, C]: the separable valid-region window, rows (along W) first, taps in ascending order, every
    product and every sum an operation of q's dtype."""
    H, W = q.shape[1], q.shape[2]
    h = torch.zeros_like(q[:, :, :W - TAPS + 1])
    for t in range(TAPS):
        h = h + w[t] * q[:, :, t:t + W - TAPS + 1]
    v = torch.zeros_like(h[:, :H - TAPS + 1])
    for t in range(TAPS):
        v = v + w[t] * h[:, t:t + H - TAPS + 1]
    return v


def ssim_map(a: torch.Tensor, b: torch.Tensor, dtype, offset: float) -> torch.Tensor:
    """The SSIM map [F, H-10, W-10, C] in `dtype`; the moments are taken of x - offset (any offset gives the same variances)."""
    w = window32().to(dtype)
    x, y = a.to(dtype) - offset, b.to(dtype) - offset
    mx, my, exx, eyy, exy = _blur(x, w), _blur(y, w), _blur(x * x, w), _blur(y * y, w), _blur(x * y, w)
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    mx, my = mx + offset, my + offset
    c1, c2 = torch.tensor(C1, dtype=dtype), torch.tensor(C2, dtype=dtype)
    num = (2.0 * (mx * my) + c1) * (2.0 * vxy + c2)
    den = ((mx * mx + my * my) + c1) * ((vx + vy) + c2)
    return num / den


def _sums(m: torch.Tensor, mask: torch.Tensor | None) -> torch.Tensor:
    """map [F, Hm, Wm, C], keep-mask [F, H, W] or None -> float64 [F, C, 2]: the sum over counted positions and their count."""
    m = m.double()
    half = TAPS // 2
    keep = (torch.ones(m.shape[:3], dtype=torch.bool) if mask is None
            else mask[:, half:half + m.shape[1], half:half + m.shape[2]])
    k = keep[..., None].expand_as(m)
    return torch.stack([torch.where(k, m, torch.zeros_like(m)).sum((1, 2)), k.double().sum((1, 2))], dim=-1)


def ssim_ref64(a, b, mask=None) -> torch.Tensor:
    return _sums(ssim_map(a, b, torch.float64, 0.0), mask)


def ssim_ref32(a, b, mask=None) -> torch.Tensor:
    return _sums(ssim_map(a, b, torch.float32, 128.0), mask)


def mean_of(sums: torch.Tensor) -> torch.Tensor:
    """[F, C, 2] -> [F, C]: sum / count, nan where nothing is counted."""
    return sums[..., 0] / sums[..., 1]
