"""References and checkers for the direct tests of the layout (ld_elem.hip), norm-form / head-split (ld_norm_*.hip) and T5 (ld_t5.hip)
kernels: tests/test_gpu_elem_kernels.py, test_gpu_norm_forms.py, test_gpu_t5_kernels.py; tests/test_kernel_ref_host.py runs every
checker here on the CPU against a correct restatement (must pass) and against deliberately wrong outputs (must fail).

Pure torch on the CPU: nothing here touches a GPU or the library.  Every reference restates an operation of the reference project
(cited by file:line in its docstring) in float64, or in the exact eager fp32 / bf16 operations where the kernel promises those bits.

Three classes of check (the GPU tests name theirs):
  A  bit-exact: `check_bits` on the WHOLE sentinel-filled buffer -- the expected buffer holds the sentinel wherever the kernel must
     not write, so a store into a border, a halo frame, a padding column or a row behind the output fails the same comparison.
  B  one rounding of an fp32 computation: `check_one_rounding` -- every element within one bf16 step of the float64 value (plus the
     fp32 noise of the computation, which the caller states), >= 99 % equal to the correctly rounded value; `check_f32` for fp32 outputs.
  C  chains with several bf16 roundings: the reference rounds where the kernel rounds and carries a per-element error bound through
     the chain with `round_bf` (one bf16 ulp per rounded intermediate, multiplied through the later factors: the scheme of
     tests/test_gpu_gemm_routes.py::_reference); `check_chain` asserts |got - ref| <= bound and >= 99 % bit-equal.
"""
import torch
import torch.nn.functional as F

from test_gpu_gemm_routes import NAN16, NAN32, _ulp        # the suite's sentinel bit patterns (quiet NaNs) and its bf16 ulp

BF = torch.bfloat16
NAN8 = 0xA5                                                # uint8 outputs: no NaN to be had, a byte the tests' data rarely ends on
MIN_EQUAL = 0.99


def bf(x):
    """float64 -> nearest bf16 -> float64."""
    return x.to(BF).double()


def bits(t):
    """The raw bits of a bf16 / fp32 tensor (int16 / int32), or the tensor itself (integer types)."""
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32) if t.dtype == torch.float32 else t


def sentinels(shape, dtype, device="cpu"):
    """A buffer of the suite's sentinel pattern, as raw bits: int16 for bf16, int32 for fp32, uint8 for bytes.  View it with
    .view(dtype) to hand it to a kernel."""
    if dtype == BF:
        return torch.full(shape, NAN16, dtype=torch.int16, device=device)
    if dtype == torch.float32:
        return torch.full(shape, NAN32, dtype=torch.int32, device=device)
    assert dtype == torch.uint8
    return torch.full(shape, NAN8, dtype=torch.uint8, device=device)


def is_sentinel(b):
    return b == {torch.int16: NAN16, torch.int32: NAN32, torch.uint8: NAN8}[b.dtype]


# ------------------------------------------------------------------------------------------------------------------------------
# checkers
# ------------------------------------------------------------------------------------------------------------------------------
def check_bits(got, want, what):
    """Class A: the two tensors (raw bits, or values whose bits are taken) are equal element for element."""
    got, want = bits(got).cpu(), bits(want).cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ, first at {i}: got bits {got[i].item():#x}, want {want[i].item():#x}")


def check_untouched(b, written, what):
    """Everything outside the boolean mask `written` still holds the sentinel."""
    b = b.cpu()
    stray = ~is_sentinel(b) & ~written
    assert not bool(stray.any()), f"{what}: {int(stray.sum())} elements outside the output were written, first at {tuple(stray.nonzero()[0].tolist())}"


def _report(what, err, bound, equal, extra=""):
    ratio = (err / bound).max().item() if err.numel() else 0.0
    print(f"{what}: worst |err| {err.max().item():.3e}, worst |err| / bound {ratio:.3f}, bit-equal to the rounded reference {equal:.6f}{extra}")
    return ratio


def check_one_rounding(got, ref64, noise, what):
    """Class B, bf16 output: got within one bf16 step of the float64 value -- ulp(ref) + noise, where `noise` is the caller's
    per-element bound on the error of the fp32 computation before the rounding (it lets a near-midpoint value take its other
    neighbour, and keeps an element that cancels to ~0 from being judged relative to itself) -- and >= 99 % of the elements equal
    to the correctly rounded value.  Returns (worst |err| / bound, equal share)."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err, bound = (g - ref64).abs(), _ulp(ref64) + noise
    equal = (g == bf(ref64)).double().mean().item()
    ratio = _report(what, err, bound, equal)
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements further than one bf16 step from the float64 value (worst ratio {ratio:.3f})"
    assert equal >= MIN_EQUAL, f"{what}: only {equal:.4f} of the elements are the correctly rounded value"
    return ratio, equal


def check_f32(got, ref64, torch32, what):
    """Class B, fp32 output (the rule of tests/test_gpu_llm_kernels.py::_ln_ref_and_bound): max |got - ref| <= 4 x the max error of
    torch's own fp32 evaluation `torch32` on the CPU (the factor covers another summation order), at least 2^-20 max |ref|."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    e_torch = (torch32.double() - ref64).abs().max().item()
    bound = max(4 * e_torch, 2.0 ** -20 * ref64.abs().max().item())
    err = (g - ref64).abs().max().item()
    print(f"{what}: max abs error {err:.3e} (torch fp32 on the CPU: {e_torch:.3e}, bound {bound:.3e})")
    assert err <= bound, (what, err, bound)
    return err / bound


def check_chain(got, ref64, bound, what):
    """Class C: |got - ref| <= bound element-wise (ref: the float64 chain rounded where the kernel rounds, bound: carried by
    round_bf) and >= 99 % of the elements bit-equal to ref.  Returns (worst |err| / bound, equal share)."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref64).abs()
    equal = (g == ref64).double().mean().item()
    ratio = _report(what, err, bound, equal, f", more than one bf16 step off: {int((err > _ulp(ref64) * 1.001).sum())}")
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements outside the carried bound (worst ratio {ratio:.3f})"
    assert equal >= MIN_EQUAL, f"{what}: only {equal:.4f} of the elements equal the reference chain"
    return ratio, equal


def round_bf(v, err):
    """One bf16 rounding point of a class-C chain: v (float64, what the kernel holds in fp32 with error <= err) -> (bf16 value,
    new error).  The fp32 value being rounded carries its own 2^-24 relative rounding; the two roundings can then land one ulp
    apart (ulp taken at the far end of the interval)."""
    err = err + 2.0 ** -24 * v.abs()
    return bf(v), err + _ulp(v.abs() + err)


# ------------------------------------------------------------------------------------------------------------------------------
# ld_elem.hip
# ------------------------------------------------------------------------------------------------------------------------------
def patchify_ref(x, sem, p):
    """ImagePatchEmbeddingMixin.word_embedding_forward's rearrangement (dit_video_concat.py:47-62: the Conv2d(C, D, p, stride p) over
    [b t] c h w reads patch (ph, pw) as the flattened [c][i][j] block) after `x + semantic_feature` in bf16 (:991).
    x fp32 [B, T, C, H, W], sem bf16 [1, T, C, H, W] or None -> bf16 [B, T*hp*wp, C*p*p]."""
    B, T, C, H, W = x.shape
    v = x.to(BF)
    if sem is not None:
        v = v + sem                                           # a bf16 add, broadcast over B
    hp, wp = H // p, W // p
    return v.view(B, T, C, hp, p, wp, p).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, T * hp * wp, C * p * p)


def fma32(a, b, c):
    """The correctly rounded fp32 fused multiply-add a*b + c of fp32 tensors (torch has none on the CPU): the product of two fp32
    numbers is exact in float64; the float64 sum is rounded to ODD (its error, from the two-sum, sets the last bit), and a value
    rounded to odd at 53 bits rounds to the nearest fp32 exactly as the unrounded one does."""
    p = a.double() * b.double()
    c = c.double().expand_as(p)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                              # s + e == p + c exactly
    i = s.contiguous().view(torch.int64)
    inexact = (e != 0) & ((i & 1) == 0)
    away = (e > 0) == (s > 0)                                  # the exact sum lies beyond s (in magnitude): the odd neighbour is the next one up
    i = torch.where(inexact, torch.where(away, i + 1, i - 1), i)
    return i.view(torch.float64).float()


def unpatchify_cfg_ref(lin, x, p, c_out, c_skip, scale, fused_last=True):
    """unpatchify (dit_video_concat.py:392-410: b (t h w) (c p q) -> b t c (h p) (w q)), Denoiser.forward's net * c_out + x * c_skip
    (denoiser.py:25-41) and the CFG combine u + scale * (c - u) (guiders.py:75-79) in eager fp32 torch operations, the scalars as fp32
    tensors as the kernel receives them.  lin bf16 [2, T*hp*wp, C*p*p] (rows 0 uncond, 1 cond), x fp32 [1, T, C, H, W].
    fused_last: the last step as ONE fma(scale, c - u, u), what ld_unpatchify_cfg computes (see its comment); False: eager torch's
    separately rounded product.  Returns fp32 [T, C, H, W]."""
    _, T, C, H, W = x.shape
    hp, wp = H // p, W // p
    e = lin.float().view(2, T, hp, wp, C, p, p).permute(0, 1, 4, 2, 5, 3, 6).reshape(2, T, C, H, W)
    co, cs, sc = (torch.tensor(v, dtype=torch.float32) for v in (c_out, c_skip, scale))
    xs = x[0] * cs
    du, dc = e[0] * co + xs, e[1] * co + xs
    d = dc - du
    return fma32(sc.expand_as(d), d, du) if fused_last else du + sc * d


def axpbypcz_ref(x, a, y=None, b=0.0, z=None, c=0.0, fused=True):
    """The sampler's elementwise updates (sampling.py:613-644,750-783) `a*x + b*y + c*z`, fp32 scalars.  fused: what ld_axpbypcz
    computes, fma(c, z, fma(b, y, a*x)); False: eager torch, every product rounded."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    v = f(a) * x
    for s, t in ((b, y), (c, z)):
        if t is not None:
            v = fma32(f(s).expand_as(t), t, v) if fused else v + f(s) * t
    return v


def timestep_embedding_ref(t, dim, max_period=10000.0):
    """timestep_embedding (sgm/modules/diffusionmodules/util.py:207-233): cos || sin of t * exp(-ln(max_period) * j / half), a zero
    column behind for odd dim.  t fp32 [B] -> (float64 reference [B, dim], absolute bound, CPU fp32 restatement as bf16).
    The bound: half a bf16 ulp of a value below 1 is at most 2^-9, and the fp32 argument t * freq carries ~8 fp32 roundings of its
    size (the product, exp's argument of size <= ln(max_period), exp itself), which cos and sin pass on with slope <= 1."""
    import math
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64)
    freq = torch.exp(-math.log(max_period) * j / half)
    arg = t.double()[:, None] * freq[None]
    ref = torch.cat([torch.cos(arg), torch.sin(arg)] + ([torch.zeros(len(t), 1, dtype=torch.float64)] if dim % 2 else []), dim=-1)
    b = 2.0 ** -9 + arg.abs() * 2.0 ** -21
    bound = torch.cat([b, b] + ([torch.zeros(len(t), 1, dtype=torch.float64)] if dim % 2 else []), dim=-1)
    f32 = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float32) / half)
    a32 = t[:, None].float() * f32[None]
    cpu = torch.cat([torch.cos(a32), torch.sin(a32)] + ([torch.zeros(len(t), 1)] if dim % 2 else []), dim=-1).to(BF)
    return ref, bound, cpu


def check_abs_rounding(got, ref64, bound, what):
    """Class B with an absolute bound (timestep embedding: the values pass through zero, where a relative rule means nothing)."""
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    err = (g - ref64).abs()
    equal = (g == bf(ref64)).double().mean().item()
    live = bound > 0
    ratio = _report(what, err[live], bound[live], equal)
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements outside the bound (worst ratio {ratio:.3f})"
    assert equal >= MIN_EQUAL, f"{what}: only {equal:.4f} of the elements are the correctly rounded value"
    return ratio, equal


def upsample_out_frames(Ti, time_up):
    return Ti if not (time_up and Ti > 1) else (2 * Ti - 1 if Ti % 2 else 2 * Ti)


def place_ref(x, mode, Cout, time_up=False):
    """What ld_place_cl puts into the interior.  x bf16 channels-last [F, Ti, Hi, Wi, Cin] -> bf16 [F, To, Ho, Wo, Cout].
    mode 0: a copy, channels zero-padded (F.pad, cp_enc_dec.py:467-468);
    mode 1: Upsample3D.forward (cp_enc_dec.py:605-627) on the [b, c, t, h, w] tensor: with compress_time and t > 1 the first frame
            apart (2-d) and the rest 3-d when t is odd, everything 3-d when even; otherwise 2-d per frame -- F.interpolate(
            scale_factor=2.0, mode="nearest") in every branch, as there;
    mode 2: torch.nn.PixelShuffle(2) per frame (vq_gan_blocks.py:41-66)."""
    Fn, Ti, Hi, Wi, Cin = x.shape
    if mode == 0:
        return F.pad(x, (0, Cout - Cin))
    v = x.float().permute(0, 4, 1, 2, 3)                      # b c t h w (bf16 values are exact in fp32; nearest only copies)
    up = lambda a: F.interpolate(a, scale_factor=2.0, mode="nearest")
    if mode == 1:
        if time_up and Ti > 1:
            if Ti % 2 == 1:
                v = torch.cat([up(v[:, :, 0])[:, :, None], up(v[:, :, 1:])], dim=2)
            else:
                v = up(v)
        else:
            v = up(v.permute(0, 2, 1, 3, 4).reshape(Fn * Ti, Cin, Hi, Wi)).view(Fn, Ti, Cin, 2 * Hi, 2 * Wi).permute(0, 2, 1, 3, 4)
    else:
        v = torch.nn.PixelShuffle(2)(v.permute(0, 2, 1, 3, 4).reshape(Fn * Ti, Cin, Hi, Wi)).view(Fn, Ti, Cout, 2 * Hi, 2 * Wi).permute(0, 2, 1, 3, 4)
    return v.permute(0, 2, 3, 4, 1).contiguous().to(BF)


def padded_expect(interior, tpad, hpad, wpad):
    """The sentinel-filled buffer [F, To + tpad, Ho + 2 hpad, Wo + 2 wpad, C] (raw bits) a placement kernel must leave: interior
    written, the tpad leading halo frames and the border cells untouched."""
    Fn, To, Ho, Wo, C = interior.shape
    b = sentinels((Fn, To + tpad, Ho + 2 * hpad, Wo + 2 * wpad, C), interior.dtype)
    b[:, tpad:, hpad:hpad + Ho, wpad:wpad + Wo] = bits(interior)
    return b


def to_uint8_ref(v):
    """_post_process_cog_video (dif_infer.py:37-49): ((v + 1) / 2).clamp(0, 1), then the uint8 frames (landiff/utils.py:327-331):
    (. * 255).clamp(0, 255).to(uint8), in fp32 on the bf16 values.  v bf16 [P, 3] -> (uint8 [P, 3], fp32 video [3, P])."""
    f = ((v.float() + 1.0) / 2.0).clamp(0.0, 1.0)
    return (f * 255.0).clamp(0.0, 255.0).to(torch.uint8), f.t().contiguous()


def finite_bf16_patterns():
    """Every finite bf16 bit pattern (65 280 values: all but the 256 with an all-ones exponent), as a bf16 tensor."""
    i = torch.arange(65536, dtype=torch.int32)
    i = i[((i >> 7) & 0xFF) != 0xFF]
    return (i - (i >= 32768).int() * 65536).to(torch.int16).view(BF)


def latent_to_cl_ref(x, T, C, H, W, Cpad, mul, src_tchw):
    """dif_infer.py:251 `1 / scale_factor * latent` on the bf16 samples, then the decoder's channels-last input with zero channels
    behind C.  x fp32 [T, C, H, W] (src_tchw) or [C, T, H, W] -> bf16 [T, H, W, Cpad]."""
    v = x.view(T, C, H, W) if src_tchw else x.view(C, T, H, W).permute(1, 0, 2, 3)
    v = (v.to(BF).float() * torch.tensor(mul, dtype=torch.float32)).to(BF)            # a bf16 multiply: fp32 product of the bf16 value, rounded
    return F.pad(v.permute(0, 2, 3, 1), (0, Cpad - C)).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# ld_norm_layer.hip, ld_norm_qkv.hip, ld_norm_group.hip
# ------------------------------------------------------------------------------------------------------------------------------
def ln_inputs(rows, D, seed, x_f32=False):
    """tests/test_gpu_llm_kernels.py::_ln_inputs: a non-zero mean (E[x^2] - mean^2 would lose its digits); bf16 weights."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g) + 3
    return (x if x_f32 else x.to(BF)), torch.randn(D, generator=g).to(BF), torch.randn(D, generator=g).to(BF)


def layernorm_ref(x, w, b, eps):
    """nn.LayerNorm (blocks.py:292-304; dit_video_concat.py:577-586) -> (float64 reference, torch's own fp32 evaluation on the CPU)."""
    D = x.shape[-1]
    wd, bd = (None, None) if w is None else (w.double(), b.double())
    ref = F.layer_norm(x.double(), (D,), wd, bd, eps)
    t32 = F.layer_norm(x.float(), (D,), None if w is None else w.float(), None if w is None else b.float(), eps)
    return ref, t32


def f32_noise(ref64, torch32):
    """The error allowed to an fp32 LayerNorm before its rounding -- the rule of tests/test_gpu_llm_kernels.py::_ln_ref_and_bound: 4 x
    the max error of torch's own fp32 evaluation on the CPU against float64 (the factor covers the other summation order: a 64-lane
    tree against torch's vectorised sum), at least 2^-20 max |ref|.  A scalar."""
    return max(4 * (torch32.double() - ref64).abs().max().item(), 2.0 ** -20 * ref64.abs().max().item())


def modulate_rows(ada, rows, rows_per_batch, text_len, off_img, off_txt, D):
    """The per-row modulation vector: batch = row // rows_per_batch, text if row % rows_per_batch < text_len (include/landiff_hip.h);
    offsets into a row of ada [B, stride]."""
    r = torch.arange(rows)
    bb = r // rows_per_batch
    txt = ((r - bb * rows_per_batch) < text_len)[:, None]
    return torch.where(txt, ada[bb, off_txt:off_txt + D], ada[bb, off_img:off_img + D]).double()


def ln_modulate_ref(x, w, b, eps, shift, scale, drop=None):
    """LayerNorm + modulate() = x * (1 + scale) + shift with every op in bf16 (dit_video_concat.py:388,601-611), rounded where
    ld_layernorm_kernel's comment says: the LayerNorm output, 1 + scale, the product, the sum.  shift, scale: float64 [rows, D] of bf16
    values.  drop names one rounding point to leave out ("ln", "one_plus", "prod"): the host test's wrong chains.
    Returns (float64 values, bound)."""
    ref, t32 = layernorm_ref(x, w, b, eps)
    err = torch.full_like(ref, f32_noise(ref, t32))
    y, err = (ref, err) if drop == "ln" else round_bf(ref, err)
    s = 1.0 + scale
    s = s if drop == "one_plus" else bf(s)                   # (exact operands: the same rounding on both sides, no error)
    m, err = (y * s, err * s.abs()) if drop == "prod" else round_bf(y * s, err * s.abs())
    return round_bf(m + shift, err)


def ln_modulate_cpu32(x, w, b, eps, shift, scale):
    """The CPU fp32 restatement of the same chain (eager torch: fp32 layer_norm, bf16 ops)."""
    y = F.layer_norm(x.float(), (x.shape[-1],), w.float(), b.float(), eps).to(BF)
    return y * (1 + scale.to(BF)) + shift.to(BF)


def split_heads(t, B, N, H):
    """[B*N, H*64] -> [B, H, N, 64]."""
    return t.view(B, N, H, 64).permute(0, 2, 1, 3)


def qkv_thirds(qkv, B, N, H):
    """qkv [B*N, 3*H*64] (thirds q | k | v, sat's SelfAttention layout) -> q, k, v as [B, H, N, 64]."""
    return tuple(split_heads(qkv[:, i * H * 64:(i + 1) * H * 64], B, N, H) for i in range(3))


def qkv_expect_bits(q, k, v, Npad, tail):
    """The three sentinel-filled flat buffers a split must leave (raw bits): Q, K [B, H, Npad, 64] with rows [N, Npad) ZERO,
    V^T [B, H, 64, Npad] with columns [N, Npad) zero, and `tail` untouched sentinel elements behind each.  q, k, v bf16 [B, H, N, 64]."""
    B, H, N, _ = q.shape
    out = []
    for t, tr in ((q, False), (k, False), (v, True)):
        full = torch.zeros(B, H, Npad, 64, dtype=BF)
        full[:, :, :N] = t
        if tr:
            full = full.transpose(2, 3).contiguous()
        out.append(torch.cat([bits(full).reshape(-1), sentinels((tail,), BF)]))
    return out


def qk_layernorm_ref(t, w, b, eps=1e-6):
    """query_layernorm / key_layernorm: LayerNorm(64, eps 1e-6) per head (dit_video_concat.py:649-653).  t bf16 [..., 64]."""
    ref, t32 = layernorm_ref(t, w, b, eps)
    return ref, t32.to(BF), f32_noise(ref, t32)


def rope_ref(t, cos, sin):
    """apply_rope (tokenizer/modules/blocks.py:172-180 -> modules/pos_emb.py:16-46): pairs (t[2e], t[2e+1]) as complex numbers times
    cos + i sin.  t bf16 [B, H, N, 64], cos / sin fp32 [N, 32] -> (float64 reference, CPU fp32 restatement as bf16, fp32 noise:
    two products and a sum)."""
    def rot(a, c, s):
        a0, a1 = a[..., 0::2], a[..., 1::2]
        return torch.stack([a0 * c - a1 * s, a0 * s + a1 * c], dim=-1).flatten(-2)
    ref = rot(t.double(), cos.double(), sin.double())
    cpu = rot(t.float(), cos, sin).to(BF)
    a = t.double().abs()
    mag = torch.stack([a[..., 0::2] * cos.double().abs() + a[..., 1::2] * sin.double().abs(),
                       a[..., 0::2] * sin.double().abs() + a[..., 1::2] * cos.double().abs()], dim=-1).flatten(-2)
    return ref, cpu, mag * 2.0 ** -22


def gn_sums_ref(x, Fn, P, C, G):
    """float64 (sum, sum of squares) of the bf16 values per (frame group, channel group), and the sums' own magnitudes (sum |x|, sum x^2)
    that an error is relative to (tests/test_gpu_gemm.py::test_conv_groupnorm_partials)."""
    v = x.double().view(Fn, P, G, C // G)
    want = torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], dim=-1)
    scale = torch.stack([v.abs().sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], dim=-1)
    return want, scale


def nearest_index_int(n_out, n_in):
    """The integer rule of ld_gn_apply_*: source index = floor(i * n_in / n_out)."""
    return (torch.arange(n_out) * n_in) // n_out


def nearest_index_torch(n_out, n_in):
    """The index F.interpolate(size=n_out, mode="nearest") takes, read off by interpolating an index ramp."""
    return F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None], size=n_out, mode="nearest")[0, 0].long()


def time_index_int(T, Tz):
    """ld_gn_apply_*'s time rule: odd T > 1 keeps the first frame apart -- frame 0 <- 0, frame t <- 1 + floor((t - 1)(Tz - 1) / (T - 1))."""
    if T > 1 and T % 2 == 1:
        t = torch.arange(T)
        return torch.where(t == 0, torch.zeros_like(t), 1 + ((t - 1) * (Tz - 1)) // max(T - 1, 1))
    return nearest_index_int(T, Tz)


def zq_gather_torch(z, T, H, W):
    """SpatialNorm3D.forward's own interpolation (cp_enc_dec.py:546-569) of z bf16 channels-last [Tz, Hz, Wz, C] to [T, H, W, C]: odd
    T > 1 splits the first frame off and interpolates both parts with size=, mode="nearest"; else one call.  (conv_y / conv_b are
    1x1x1, so gathering their low-resolution outputs equals convolving the gathered zq.)
    torch's nearest rule multiplies by a float scale; it equals the kernel's exact integer rule for every ratio the pipeline
    produces (1, 2, 4, 8 and the odd-T time rule: tests/test_kernel_ref_host.py) but not everywhere -- in 2 -> out 82 and 3 -> 123
    differ -- so tests keep to ratios where nearest_index_int == nearest_index_torch and assert that."""
    v = z.float().permute(3, 0, 1, 2)[None]                   # 1 c t h w
    if T > 1 and T % 2 == 1:
        v = torch.cat([F.interpolate(v[:, :, :1], size=(1, H, W), mode="nearest"),
                       F.interpolate(v[:, :, 1:], size=(T - 1, H, W), mode="nearest")], dim=2)
    else:
        v = F.interpolate(v, size=(T, H, W), mode="nearest")
    return v[0].permute(1, 2, 3, 0).to(BF)


def zq_gather_int(z, T, H, W, first_frame_rule=True):
    """The same gather by the kernel's integer rules (first_frame_rule=False: the wrong kernel of the host test)."""
    Tz, Hz, Wz, _ = z.shape
    ti = time_index_int(T, Tz) if first_frame_rule else nearest_index_int(T, Tz)
    return z[ti][:, nearest_index_int(H, Hz)][:, :, nearest_index_int(W, Wz)]


def gn_apply_ref(x, sums, gamma, beta, Fn, T, H, W, C, G, eps, zy=None, zb=None, swish=True, drop=None):
    """GroupNorm (torch.nn.GroupNorm(32, eps 1e-6) in Normalize, vq_gan_blocks.py:29-38, and in SpatialNorm3D) -> bf16;
    norm_f * conv_y(zq) + conv_b(zq) (cp_enc_dec.py:546-569) and x * sigmoid(x) (:67-69) in bf16 steps, rounded where
    ld_gn_apply_*'s comments say: the GroupNorm output, the product, the sum, the sigmoid, the final product.
    x bf16 [F*T, H, W, C], sums float64 [F, G, 2] (the statistics handed to the kernel), zy / zb bf16 [T, H, W, C] ALREADY gathered.
    drop ("gn", "prod", "sig"): one rounding point left out, for the host test.  Returns (float64 values [F, T, H, W, C], bound)."""
    cpg = C // G
    n = T * H * W * cpg
    mean = (sums[..., 0] / n)
    var = (sums[..., 1] / n - mean * mean).clamp(min=0)
    rstd = torch.rsqrt(var.float().double() + eps)           # (the kernel casts the variance to fp32 first; the cast is inside the bound)
    ch = lambda s: s.repeat_interleave(cpg, dim=1)[:, None, None, None, :]      # [F, G] -> [F, 1, 1, 1, C]
    xv = x.double().view(Fn, T, H, W, C)
    g64, b64 = gamma.double(), beta.double()
    v = (xv - ch(mean)) * ch(rstd) * g64 + b64
    # fp32: the mean's cast (2^-24 |mean|), a difference, rsqrt (1 ulp), two products and a sum -- 2^-21 of the terms' magnitudes
    err = ((xv.abs() + ch(mean).abs()) * ch(rstd) * g64.abs() + b64.abs()) * 2.0 ** -21
    y, err = (v, err) if drop == "gn" else round_bf(v, err)
    if zy is not None:
        zyd, zbd = zy.double()[None], zb.double()[None]
        y, err = (y * zyd, err * zyd.abs()) if drop == "prod" else round_bf(y * zyd, err * zyd.abs())
        y, err = round_bf(y + zbd, err)
    if swish:
        sg = torch.sigmoid(y)
        # the sigmoid's slope is at most 1/4; exp(-y) as exp2(-y log2 e) carries |y| roundings of its size from the rounded product, the
        # hardware exp2 and reciprocal an ulp or two each, the sum one
        esg = 0.25 * err + (y.abs() + 6) * 2.0 ** -24 * sg
        sgb, esg = (sg, esg) if drop == "sig" else round_bf(sg, esg)
        y, err = round_bf(y * sgb, err * sgb.abs() + y.abs() * esg)
    return y, err


def gn_apply_cpu32(x, sums, gamma, beta, Fn, T, H, W, C, G, eps, zy=None, zb=None, swish=True):
    """The CPU fp32 / bf16-op restatement of the chain (statistics from the same sums)."""
    cpg = C // G
    n = T * H * W * cpg
    mean = sums[..., 0] / n
    var = (sums[..., 1] / n - mean * mean).clamp(min=0)
    ch = lambda s: s.repeat_interleave(cpg, dim=1)[:, None, None, None, :]
    rstd = torch.rsqrt(var.float() + eps)
    y = ((x.float().view(Fn, T, H, W, C) - ch(mean.float())) * ch(rstd) * gamma.float() + beta.float()).to(BF)
    if zy is not None:
        y = y * zy[None] + zb[None]
    if swish:
        y = y * torch.sigmoid(y.float()).to(BF)
    return y


# ------------------------------------------------------------------------------------------------------------------------------
# ld_t5.hip
# ------------------------------------------------------------------------------------------------------------------------------
def t5_rmsnorm_ref(x, w, eps, drop=None):
    """T5LayerNorm (transformers modeling_t5.py): variance = mean(x^2) in fp32, x * rsqrt(variance + eps) rounded to the weight's
    bf16, weight * that rounded again.  x bf16 [rows, D], w bf16 [D] -> (float64 values, bound).  drop="inner": without the first
    rounding (host test)."""
    xd = x.double()
    v = xd * torch.rsqrt(xd.square().mean(-1, keepdim=True) + eps)
    err = v.abs() * 2.0 ** -20                                # fp32 sum of squares over D <= 4096 (~14 additions deep), a division, rsqrt, a product
    n, err = (v, err) if drop == "inner" else round_bf(v, err)
    wd = w.double()
    return round_bf(wd * n, err * wd.abs())


def t5_rmsnorm_cpu32(x, w, eps):
    xf = x.float()
    return w * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(BF)


def t5_attn_ref(q, k, v, bias_table, bucket, exact_scores=True, drop=None):
    """T5Attention.forward of the bf16 HF module (transformers modeling_t5.py; called from text_encoder.py:36-42 and
    encoders/modules.py:249-292): scores = q k^T (bf16 matmul output, no 1/sqrt(d)), + position_bias[bucket(j - i)] (a bf16 add),
    softmax in fp32 cast back to bf16, probabilities @ v with fp32 accumulation -> bf16.
    q, k, v bf16 [N, H, 64], bias_table bf16 [buckets, H], bucket int [2N - 1] -> (float64 values [N, H, 64], bound).
    exact_scores asserts the premise of the GPU test: q.k and q.k + bias are bf16 numbers, so that the scores carry no error and a
    score cannot flip (one flipped bf16 score of size ~4 moves a probability by ~12 %).  drop="prob": probabilities left unrounded."""
    N, H, _ = q.shape
    qd, kd, vd = q.double().permute(1, 0, 2), k.double().permute(1, 0, 2), v.double().permute(1, 0, 2)
    s = qd @ kd.transpose(1, 2)                               # [H, N, N]
    i = torch.arange(N)
    rel = (i[None, :] - i[:, None] + N - 1)
    bias = bias_table.double()[bucket.long()[rel]].permute(2, 0, 1)
    if exact_scores:
        assert torch.equal(s, bf(s)) and torch.equal(s + bias, bf(s + bias)), "premise: the scores are not exact in bf16"
    s = bf(bf(s) + bias)
    p = torch.softmax(s, dim=-1)
    # fp32 softmax: exp (hardware approximation, ~2 ulp) of an exact difference, a sum of <= 512 positive terms, a reciprocal, a product
    ep = p * 2.0 ** -19
    pb, ep = (p, ep) if drop == "prob" else round_bf(p, ep)
    o = pb @ vd
    eo = ep @ vd.abs() + (pb @ vd.abs()) * (N + 8) * 2.0 ** -24
    o, eo = round_bf(o, eo)
    return o.permute(1, 0, 2), eo.permute(1, 0, 2)


def t5_attn_cpu32(q, k, v, bias_table, bucket):
    """The CPU restatement in eager torch ops of the same dtypes (fp32 softmax, bf16 probabilities, fp32 accumulation)."""
    N, H, _ = q.shape
    s = (q.float().permute(1, 0, 2) @ k.float().permute(1, 2, 0)).to(BF)
    i = torch.arange(N)
    s = s + bias_table[bucket.long()[i[None, :] - i[:, None] + N - 1]].permute(2, 0, 1)
    p = torch.softmax(s.float(), dim=-1).to(BF)
    return (p.float() @ v.float().permute(1, 0, 2)).to(BF).permute(1, 0, 2)


def t5_exact_operands(N, H, num_buckets, seed):
    """Operands whose scores are exact in bf16: q, k sparse {-1, 0, 1} (~6 non-zero products per score: |q.k| stays far below 256,
    the integers bf16 holds), bias a multiple of 0.5 in [-4, 4]; v ~ N(0, 1).  Returns q, k, v bf16 [N, H, 64], bias_table bf16 [buckets, H]."""
    g = torch.Generator().manual_seed(seed)
    tern = lambda: (torch.randint(-1, 2, (N, H, 64), generator=g) * (torch.rand(N, H, 64, generator=g) < 0.45)).to(BF)
    q, k = tern(), tern()
    v = torch.randn(N, H, 64, generator=g).to(BF)
    bias = (torch.randint(-8, 9, (num_buckets, H), generator=g) * 0.5).to(BF)
    return q, k, v, bias
