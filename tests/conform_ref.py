"""Float64 restatement of the conform stage's resampling for the tests (TEST INFRASTRUCTURE): PyTorch's antialias weight tables,
written out tap by tap in Python; the resize as two matrix products; the conservative mask rule.  Nothing here imports
landiff_amd.conform: the product's tables are compared against these, and these against F.interpolate(antialias=True)."""
import numpy as np
import torch

A = -0.5


def _f(x: float, filt: str) -> float:
    x = abs(x)
    if filt == "bilinear":
        return 1.0 - x if x < 1.0 else 0.0
    if x < 1.0:
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    if x < 2.0:
        return A * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


def tables(n_in: int, n_out: int, filt: str):
    """-> (lo [n_out], hi [n_out], weights: list of n_out lists): output i is sum_j w[i][j - lo[i]] * in[j], j in [lo[i], hi[i])."""
    half = 1.0 if filt == "bilinear" else 2.0
    scale = n_in / n_out
    support, inv = (half * scale, 1.0 / scale) if scale >= 1.0 else (half, 1.0)
    lo, hi, ws = [], [], []
    for i in range(n_out):
        c = scale * (i + 0.5)
        a, b = max(0, int(c - support + 0.5)), min(n_in, int(c + support + 0.5))
        raw = [_f((j - c + 0.5) * inv, filt) for j in range(a, b)]
        tot = sum(raw)
        lo.append(a); hi.append(b); ws.append([v / tot for v in raw])
    return lo, hi, ws


def matrix(n_in: int, n_out: int, filt: str) -> torch.Tensor:
    """The axis as a float64 [n_out, n_in] matrix."""
    lo, hi, ws = tables(n_in, n_out, filt)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        m[i, lo[i]:hi[i]] = torch.tensor(ws[i], dtype=torch.float64)
    return m


def resize_ref(src: torch.Tensor, Ho: int, Wo: int, filt: str, box=None, frame_idx=None) -> torch.Tensor:
    """uint8 [F, H, W, C] -> float64 [n, Ho, Wo, C], unrounded: My @ crop(src[frame_idx]) @ Mx^T per frame and channel."""
    y0, x0, hc, wc = box or (0, 0, src.shape[1], src.shape[2])
    idx = list(range(src.shape[0])) if frame_idx is None else list(frame_idx)
    x = src[idx][:, y0:y0 + hc, x0:x0 + wc].double()
    my, mx = matrix(hc, Ho, filt), matrix(wc, Wo, filt)
    return torch.einsum("oh,fhwc,pw->fopc", my, x, mx)


def quantize(v: torch.Tensor) -> torch.Tensor:
    """The one rounding: clamp(round-half-even(v), 0, 255) as uint8."""
    return torch.clamp(torch.round(v), 0, 255).to(torch.uint8)


def eps_bound(hc: int, wc: int, Ho: int, Wo: int, filt: str) -> float:
    """The fp32 error bound of the issue: (2 (t_y + t_x) + 4) 2^-24 255 L_y L_x, t the largest tap count of an axis and L the largest
    sum of |w| of a row -- weights rounded to fp32 and a (t_y + t_x)-term fp32 accumulation."""
    out = []
    for n_in, n_out in ((hc, Ho), (wc, Wo)):
        lo, hi, ws = tables(n_in, n_out, filt)
        out.append((max(b - a for a, b in zip(lo, hi)), max(sum(abs(v) for v in w) for w in ws)))
    (ty, Ly), (tx, Lx) = out
    return (2 * (ty + tx) + 4) * 2.0 ** -24 * 255.0 * Ly * Lx


def mask_ref(mask: torch.Tensor, Ho: int, Wo: int, filt: str, box=None, frame_idx=None) -> torch.Tensor:
    """[F, H, W] (non-zero = keep) -> uint8 [n, Ho, Wo]: 1 iff every source pixel of the window [lo_y, hi_y) x [lo_x, hi_x) is non-zero."""
    y0, x0, hc, wc = box or (0, 0, mask.shape[1], mask.shape[2])
    idx = list(range(mask.shape[0])) if frame_idx is None else list(frame_idx)
    m = (mask[idx][:, y0:y0 + hc, x0:x0 + wc] != 0).numpy()
    ly, hy, _ = tables(hc, Ho, filt)
    lx, hx, _ = tables(wc, Wo, filt)
    cols = np.stack([m[:, :, lx[j]:hx[j]].all(axis=2) for j in range(Wo)], axis=2)            # [n, hc, Wo]
    out = np.stack([cols[:, ly[i]:hy[i], :].all(axis=1) for i in range(Ho)], axis=1)          # [n, Ho, Wo]
    return torch.from_numpy(out.astype(np.uint8))
