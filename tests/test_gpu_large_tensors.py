"""The convolution, GroupNorm and VAE-encoder kernels on tensors past 2 GiB, 4 GiB and 2^31 elements: the sizes a 49-frame
480 x 720 encode (extend_video's clip) reaches.  Random data throughout, so that a row read from the wrong place is an O(1)
error, and every reference is computed without torch touching a tensor of 2^31 elements or more: inputs are filled, compared
and summed per frame or per chunk, and the convolution reference gathers each sampled output row's receptive field in float64."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
CHUNK = 1 << 28                     # elements per torch op on a large tensor


def _lib():
    from landiff_amd import _lib
    return _lib.load()


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def fill_randn(t, seed, scale=1.0, mean=0.0):
    """t.normal_() in chunks of CHUNK elements (views of the flat tensor)."""
    g = torch.Generator(device=t.device).manual_seed(seed)
    for c in t.view(-1).split(CHUNK):
        c.normal_(mean, scale, generator=g)
    return t


def equal_chunked(a, b):
    return a.shape == b.shape and all(torch.equal(x, y) for x, y in zip(a.reshape(-1).split(CHUNK), b.reshape(-1).split(CHUNK)))


def _by_frame(rows, HW):
    """rows (cpu int64, sorted) -> [(frame, positions in rows, row index within the frame)]."""
    t = rows // HW
    out = []
    for f in torch.unique(t).tolist():
        sel = (t == f).nonzero().flatten()
        out.append((f, sel, rows[sel] - f * HW))
    return out


def gather_rows(x2d, rows, HW):
    """Rows of a [M, C] tensor, float64 on the device: indexed one frame of HW rows at a time (a view, small index space)."""
    out = torch.empty(len(rows), x2d.shape[1], dtype=torch.float64, device=x2d.device)
    for f, sel, loc in _by_frame(rows, HW):
        out[sel.to(x2d.device)] = x2d.narrow(0, f * HW, HW)[loc.to(x2d.device)].double()
    return out


def boundary_rows(T, H, W, kT, kH, kW, Cin):
    """Output rows whose receptive field holds the padded input element at byte offset 2^31, 2^32 or 2^33 (those inside)."""
    Tp, Hp, Wp = T + kT - 1, H + kH - 1, W + kW - 1
    total = Tp * Hp * Wp * Cin
    rows = []
    for byte in (1 << 31, 1 << 32, 1 << 33):
        e = byte // 2
        if e >= total:
            continue
        pix = e // Cin
        tp, hp, wp = pix // (Hp * Wp), (pix // Wp) % Hp, pix % Wp
        here = [((tp - dt) * H + hp - dh) * W + wp - dw for dt in range(kT) for dh in range(kH) for dw in range(kW)
                if 0 <= tp - dt < T and 0 <= hp - dh < H and 0 <= wp - dw < W]
        assert here, (byte, tp, hp, wp)
        rows += here
    return rows


def sample_rows(T, H, W, kT, kH, kW, Cin, seed, n_random=2048):
    """The boundary rows, the first and last 256 rows (tile edges) and n_random seeded random rows, sorted and unique."""
    M = T * H * W
    g = torch.Generator().manual_seed(seed)
    rows = (boundary_rows(T, H, W, kT, kH, kW, Cin) + list(range(256)) + list(range(M - 256, M))
            + torch.randint(0, M, (n_random,), generator=g).tolist())
    return torch.tensor(sorted(set(rows)), dtype=torch.int64)


def conv_rows_ref(xp, w, rows, H, W, bias=None):
    """Output rows `rows` of the channels-last conv (ld_conv_cl_bf16's operation) in float64 from their receptive fields:
    each row gathers its kT * kH * kW taps x Cin channels from the padded input [Tp][Hp][Wp][Cin] and takes the dot product
    with the weight [Cout][kT][kH][kW][Cin] flattened in the same [dt][dh][dw][c] order.  -> (conv + bias, sum of |products|)."""
    Cout, kT, kH, kW, Cin = w.shape
    _, Hp, Wp, _ = xp.shape
    dev = xp.device
    HW = H * W
    taps = ((torch.arange(kH)[:, None, None] * Wp + torch.arange(kW)[None, :, None]) * Cin
            + torch.arange(Cin)[None, None, :]).reshape(-1).to(dev)                       # within one input frame
    A = torch.empty(len(rows), kT * kH * kW * Cin, dtype=torch.float64, device=dev)
    span = kH * kW * Cin
    for f, sel, loc in _by_frame(rows, HW):
        base = ((loc // W) * Wp + loc % W) * Cin
        idx = base.to(dev)[:, None] + taps[None, :]
        sel = sel.to(dev)
        for dt in range(kT):
            A[sel, dt * span:(dt + 1) * span] = xp[f + dt].reshape(-1)[idx].double()
    wf = w.reshape(Cout, -1).double()
    ref = A @ wf.t()
    mag = A.abs() @ wf.abs().t()
    if bias is not None:
        ref += bias.double()
        mag += bias.double().abs()
    return ref, mag


def check_conv_rows(out, xp, w, T, H, W, rows, bias=None, resid=None):
    """The sampled rows of a bf16 conv output against conv_rows_ref: the kernel rounds conv + bias to bf16 once, and again
    after the residual add; its fp32 sums may differ from exact by a small fraction of the sum of |products|."""
    c, mag = conv_rows_ref(xp, w, rows, H, W, bias)
    got = gather_rows(out, rows, H * W)
    y = c + (gather_rows(resid, rows, H * W) if resid is not None else 0)
    tol = 2.0 ** -8 * (y.abs() + (c.abs() if resid is not None else 0)) + 2e-5 * mag
    bad = (got - y).abs() > tol
    if bad.any():
        i, j = [int(v) for v in bad.nonzero()[0]]
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} sampled values off; first: row {int(rows[i])} channel {j}: "
                             f"got {got[i, j].item():.5f}, want {y[i, j].item():.5f} (tol {tol[i, j].item():.2e})")


def conv_case(cuda, T, H, W, Cin, Cout, kT, kH, kW, seed):
    Tp, Hp, Wp = T + kT - 1, H + kH - 1, W + kW - 1
    xp = fill_randn(torch.empty(Tp, Hp, Wp, Cin, device=cuda, dtype=BF), seed)
    K = kT * kH * kW * Cin
    g = torch.Generator(device=cuda).manual_seed(seed + 1)
    w = (torch.randn(Cout, kT, kH, kW, Cin, device=cuda, generator=g) * K ** -0.5).to(BF)
    bias = torch.randn(Cout, device=cuda, generator=g).to(BF)
    return xp, w, bias


def check_slice_identity(out, xp, w, T, H, W, **epi):
    """The last two output frames of the big conv == a conv over the last 2 + kT - 1 input frames (a small problem on another
    route: the routes are bit-identical)."""
    from landiff_amd import ops
    kT = w.shape[1]
    HW = H * W
    small_xp = xp[T - 2:T + kT - 1].contiguous()
    small = ops.conv_cl(small_xp, w, 2, H, W, **epi)
    assert torch.equal(small, out[(T - 2) * HW:]), "last two frames differ from the same conv run on their own window"


LARGE_CONVS = [
    # id, (T, H, W, Cin, Cout, kT, kH, kW), route, padded input GiB (lower bound): the encoder's conv_in and level-0
    # downsample at 49 x 480 x 720, then 480 x 720 Cin = Cout = 256 convs on each side of the 2 GiB route switch
    ("conv_in", (49, 480, 720, 64, 128, 3, 3, 3), 0, 2.1),
    ("level0_downsample", (25, 240, 360, 512, 128, 1, 3, 3), 0, 2.08),
    ("8phase_below_2GiB", (10, 480, 720, 256, 256, 3, 3, 3), 2, 1.98),
    ("route1_above_2GiB", (11, 480, 720, 256, 256, 3, 3, 3), 1, 2.15),
    ("route1_near_2p32_elements", (45, 480, 720, 256, 256, 3, 3, 3), 1, 7.79),
]


@pytest.mark.parametrize("shape,route,gib", [c[1:] for c in LARGE_CONVS], ids=[c[0] for c in LARGE_CONVS])
def test_large_conv_sampled_rows(cuda, shape, route, gib):
    """A conv whose padded input lies just below (the 8-phase kernel's raw buffer descriptor) or past 2 GiB (and 4 GiB /
    2^31 elements for T 45) against the float64 receptive-field reference on its boundary, edge and random rows, then the
    slice identity on its last two frames."""
    from landiff_amd import ops
    T, H, W, Cin, Cout, kT, kH, kW = shape
    assert _lib().ld_conv_route(*shape) == route
    nbytes = (T + kT - 1) * (H + kH - 1) * (W + kW - 1) * Cin * 2
    assert gib < nbytes / 2 ** 30 < gib + 0.05
    xp, w, bias = conv_case(cuda, T, H, W, Cin, Cout, kT, kH, kW, seed=T * 1000 + Cin)
    out = ops.conv_cl(xp, w, T, H, W, bias=bias)
    check_conv_rows(out, xp, w, T, H, W, sample_rows(T, H, W, kT, kH, kW, Cin, seed=T), bias=bias)
    check_slice_identity(out, xp, w, T, H, W, bias=bias)
    del xp, out
    _free()


def _group_sums(x2d, G, chunk_rows=1 << 20):
    """float64 (sum, sum of squares) and sum of |x| per channel group of a [M, C] tensor, in chunks of rows."""
    C = x2d.shape[1]
    s = torch.zeros(G, 3, dtype=torch.float64, device=x2d.device)
    for c in x2d.split(chunk_rows):
        d = c.double().view(-1, G, C // G)
        s[:, 0] += d.sum(dim=(0, 2)); s[:, 1] += (d * d).sum(dim=(0, 2)); s[:, 2] += d.abs().sum(dim=(0, 2))
    return s


def test_encoder_level0_conv_past_4GiB_with_groupnorm_partials(cuda):
    """The encoder's level-0 resblock conv at 49 x 480 x 720 (Cin = Cout = 128, bias + residual): a 4.2 GiB window of 2.27e9
    elements, 2.17e9 output elements, on the 128 x 128 two-stage kernel (32-bit element offsets up to 2.27e9).  The
    GroupNorm-partials launch equals the plain launch bit for bit; its statistics match float64 sums over the output and the
    direct statistics pass over the 2.17e9 elements."""
    from landiff_amd import ops
    T, H, W, C, G = 49, 480, 720, 128, 32
    M = T * H * W
    assert _lib().ld_conv_route(T, H, W, C, C, 3, 3, 3) == 0
    assert (T + 2) * 482 * 722 * C * 2 > 2 ** 32 and M * C > 2 ** 31
    xp, w, bias = conv_case(cuda, T, H, W, C, C, 3, 3, 3, seed=4901)
    resid = fill_randn(torch.empty(M, C, device=cuda, dtype=BF), 4902)
    out, part = ops.conv_cl(xp, w, T, H, W, gn_partials=True, bias=bias, resid=resid)
    check_conv_rows(out, xp, w, T, H, W, sample_rows(T, H, W, 3, 3, 3, C, seed=49), bias=bias, resid=resid)
    check_slice_identity(out, xp, w, T, H, W, bias=bias, resid=resid[(T - 2) * H * W:])
    plain = ops.conv_cl(xp, w, T, H, W, bias=bias, resid=resid)
    assert equal_chunked(out, plain)
    del plain, xp, resid
    _free()
    stats = torch.full((1, G, 2), float("nan"), device=cuda, dtype=torch.float64)
    ops.groupnorm_stats_from_conv(part, stats, M, C, G)
    want = _group_sums(out, G)
    scale = torch.stack([want[:, 2], want[:, 1]], dim=-1)          # the sums' own magnitude (sum of |x|: the mean may cancel)
    assert ((stats[0] - want[:, :2]).abs() / scale).max().item() < 2e-6
    direct = torch.full((1, G, 2), float("nan"), device=cuda, dtype=torch.float64)
    ops.groupnorm_stats(out, direct, 1, M, C, G)
    assert ((direct[0] - want[:, :2]).abs() / scale).max().item() < 2e-6
    assert ((stats[0] - direct[0]).abs() / scale).max().item() < 2e-6
    del out, part
    _free()


ROUTE_SNIPPET = r"""
import sys, hashlib, torch
sys.path.insert(0, %r)
from landiff_amd import _lib, ops
T, H, W, C = 2, 256, 264, 256
assert _lib.load().ld_conv_route(T, H, W, C, C, 3, 3, 3) == int(sys.argv[1]), _lib.load().ld_conv_route(T, H, W, C, C, 3, 3, 3)
g = torch.Generator(device="cuda").manual_seed(7)
xp = torch.randn(T + 2, H + 2, W + 2, C, device="cuda", generator=g).to(torch.bfloat16)
w = (torch.randn(C, 3, 3, 3, C, device="cuda", generator=g) * (27 * C) ** -0.5).to(torch.bfloat16)
bias = torch.randn(C, device="cuda", generator=g).to(torch.bfloat16)
resid = torch.randn(T * H * W, C, device="cuda", generator=g).to(torch.bfloat16)
for epi in (dict(bias=bias), dict(bias=bias, resid=resid)):
    h = hashlib.sha256()
    h.update(ops.conv_cl(xp, w, T, H, W, **epi).cpu().view(torch.int16).numpy().tobytes())
    out, part = ops.conv_cl(xp, w, T, H, W, gn_partials=True, **epi)
    h.update(out.cpu().view(torch.int16).numpy().tobytes()); h.update(part.cpu().numpy().tobytes())
    print("HASH", len(epi), h.hexdigest())
""" % ROOT


def test_conv_routes_bit_identical():
    """The three GEMM routes of one conv (8-phase 256 x 256, 128 x 128 two-stage, 256 x 256 two-stage -- each its own process:
    the launcher reads LD_GEMM_TILE / LD_GEMM_8P once), with and without the residual and GroupNorm partials: same bits."""
    hashes = []
    for env, route in (({}, 2), ({"LD_GEMM_TILE": "1"}, 0), ({"LD_GEMM_TILE": "3", "LD_GEMM_8P": "0"}, 1)):
        e = dict(os.environ)
        for k in ("LD_GEMM_TILE", "LD_GEMM_8P", "LD_TUNING"):
            e.pop(k, None)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", ROUTE_SNIPPET, str(route)], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        hashes.append([l for l in r.stdout.splitlines() if l.startswith("HASH")])
        assert len(hashes[-1]) == 2
    assert all(h == hashes[0] for h in hashes[1:]), hashes


def test_groupnorm_apply_past_2p31_elements(cuda):
    """GroupNorm + swish of the encoder's 49-frame level-0 activation (2.17e9 elements) into its conv window (tpad 2, hpad 1,
    wpad 1): the statistics pass against float64 sums, sampled rows at the start, around element 2^31 and at the end against the
    torch restatement of GN_SNIPPET (tests/test_gpu_variants.py) within two bf16 steps, border and halo frames untouched."""
    from landiff_amd import ops
    T, H, W, C, G = 49, 480, 720, 128, 32
    M, HW = T * H * W, H * W
    x = fill_randn(torch.empty(M, C, device=cuda, dtype=BF), 77, scale=1.5, mean=0.3)
    gen = torch.Generator(device=cuda).manual_seed(78)
    gamma = (1 + 0.2 * torch.randn(C, device=cuda, generator=gen)).to(BF)
    beta = (0.2 * torch.randn(C, device=cuda, generator=gen)).to(BF)
    stats = torch.full((1, G, 2), float("nan"), device=cuda, dtype=torch.float64)
    ops.groupnorm_stats(x, stats, 1, M, C, G)
    want = _group_sums(x, G)
    scale = torch.stack([want[:, 2], want[:, 1]], dim=-1)
    assert ((stats[0] - want[:, :2]).abs() / scale).max().item() < 2e-6
    SENT = -7.0                                                          # below swish's minimum
    out = torch.empty(T + 2, H + 2, W + 2, C, device=cuda, dtype=BF)
    for f in out:
        f.fill_(SENT)
    ops.groupnorm_apply(x, out, stats, gamma, beta, 1, T, H, W, C, G, tpad=2, hpad=1, wpad=1, swish=True, eps=1e-6)
    mid = (1 << 31) // C
    g = torch.Generator().manual_seed(79)
    rows = torch.tensor(sorted(set(list(range(4096)) + list(range(mid - 4096, mid + 4096)) + list(range(M - 4096, M))
                                   + torch.randint(0, M, (4096,), generator=g).tolist())), dtype=torch.int64)
    n = M * (C // G)
    mu = (want[:, 0] / n).float()
    var = (want[:, 1] / n - (want[:, 0] / n) ** 2).float()
    xs = gather_rows(x, rows, HW).float().view(-1, G, C // G)
    y = (((xs - mu[:, None]) * torch.rsqrt(var[:, None] + 1e-6)).view(-1, C) * gamma.float() + beta.float()).to(BF)
    y = (y * torch.sigmoid(y)).float()
    got = torch.empty_like(y)
    for f, sel, loc in _by_frame(rows, HW):
        got[sel.to(cuda)] = out[f + 2, 1:1 + H, 1:1 + W].reshape(HW, C)[loc.to(cuda)].float()
    err = ((got - y).abs() / (y.abs() + 1.0)).max().item()
    assert err < 2 ** -6, err
    for t in range(T + 2):
        f = out[t]
        if t < 2:
            assert (f == SENT).all(), f"halo frame {t} written"
        else:
            for edge in (f[0], f[-1], f[:, 0], f[:, -1]):
                assert (edge == SENT).all(), f"border of frame {t} written"
            assert not (f[1:-1, 1:-1] == SENT).any(), f"interior of frame {t} not written"
    del x, out
    _free()


def test_encoder_layout_kernels_49_frames(cuda):
    """ld_vae_enc_place_input on a 49 x 480 x 720 clip (a 2.27e9-byte window) and ld_vae_enc_downsample on the 49-frame
    level-0 activation (2.17e9 elements in, time pool + space-to-depth out), bit for bit against the torch restatements."""
    from landiff_amd import ops
    from vae_encoder_ref import space_to_depth
    F, H, W = 49, 480, 720
    g = torch.Generator(device=cuda).manual_seed(5)
    frames = torch.randint(0, 256, (F, H, W, 3), device=cuda, generator=g, dtype=torch.uint8)
    xp = torch.empty(F + 2, H + 2, W + 2, 64, device=cuda, dtype=BF)
    for f in xp:
        f.fill_(-1e4)                                                    # every element must be overwritten
    ops.vae_enc_place_input(frames, xp)
    lut = (torch.arange(256, dtype=torch.float32) / 127.5 - 1.0).to(BF).to(cuda)     # the test_gpu_vae_encoder arithmetic
    for t in range(F + 2):
        want = torch.zeros(H + 2, W + 2, 64, device=cuda, dtype=BF)
        want[1:-1, 1:-1, :3] = lut[frames[max(t - 2, 0)].long()]
        assert torch.equal(xp[t], want), f"padded frame {t}"
    del xp, frames
    _free()
    C = 128
    h = fill_randn(torch.empty(F * H * W, C, device=cuda, dtype=BF), 6)
    assert h.numel() > 2 ** 31
    To = ops.vae_enc_downsample_out_frames(F, True)
    out = torch.empty(To, H // 2 + 2, W // 2 + 2, 4 * C, device=cuda, dtype=BF)
    for f in out:
        f.fill_(-1e4)
    ops.vae_enc_downsample(h, out, F, H, W, C, True)
    hf = h.view(F, H, W, C)
    for j in range(To):                                                  # odd F: frame 0 kept, then pairs
        src = hf[0] if j == 0 else ((hf[2 * j - 1].float() + hf[2 * j].float()) * 0.5).to(BF)
        assert torch.equal(out[j], space_to_depth(src)), f"output frame {j}"
    del h, out
    _free()
