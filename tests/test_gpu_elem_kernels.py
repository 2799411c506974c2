"""The layout / elementwise kernels of ld_elem.hip, each against a plain reference of the same operation (tests/kernel_ref.py), through
landiff_amd.ops, at small non-square shapes, with every output inside a buffer of NaN sentinels that is compared as a whole: a
transposed patch index, a wrong first-frame rule, a store into a border, a halo frame or behind the output fails.

Classes (kernel_ref's docstring): A, bit-exact, for everything here except ld_timestep_embedding (B, with an absolute bound).
ld_unpatchify_cfg and ld_axpbypcz are bit-exact against what their comments state -- eager fp32 torch operations up to a LAST step that
is one fused multiply-add per remaining term -- and are also compared with fully unfused eager torch, which they meet to a rounding:
the fusion is what these kernels have always compiled to, the other kernels of the sampler step (ld_unpatchify_cfg_keep) restate it to
stay bit-identical with it, and the kernels now spell it out instead of leaving it to the compiler's contraction.

Measured on an MI355X: every class-A comparison equal; ld_unpatchify_cfg differs from unfused eager torch in 177 of 720 elements at scale
6.5 (0 at scale 1 and, on this data, with c_skip 0), ld_axpbypcz in 29 % (x + y) and 37 % (x + y + z) of 4 194 561 elements, none with x
alone; ld_timestep_embedding: worst |err| / bound 0.999 (a half-ulp rounding of a value in [0.5, 1) with a small argument), correctly
rounded share 0.9969 ... 0.9984 at B = 5 and 0.9922 (1 of 128) / 0.99375 (12 of 1920) for t = 999 alone, the hardest single row."""
import pytest
import torch

import kernel_ref as kr
from kernel_ref import BF
from landiff_amd.config import PipelineConfig

pytestmark = pytest.mark.gpu

TAIL = 64                      # sentinel elements behind (and, where stated, in front of) a dense output


def _flat(n, dtype, cuda, front=0):
    """A flat sentinel buffer of front + n + TAIL elements -> (raw bits, the n-element view to hand to the kernel)."""
    b = kr.sentinels((front + n + TAIL,), dtype, cuda)
    return b, b.view(dtype)[front:front + n]


def _expect_flat(ref, front=0):
    return torch.cat([kr.sentinels((front,), ref.dtype), kr.bits(ref.contiguous()).reshape(-1), kr.sentinels((TAIL,), ref.dtype)])


# ---- patchify ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sem", [True, False], ids=["sem", "nosem"])
@pytest.mark.parametrize("shape", [(2, 3, 4, 6, 10), (1, 2, 16, 8, 12)], ids=lambda s: "x".join(map(str, s)))
def test_patchify(cuda, shape, with_sem):
    """Class A: a bf16 cast, a bf16 add and a permutation (dit_video_concat.py:47-62,991)."""
    from landiff_amd import ops
    B, T, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    sem = torch.randn(1, T, C, H, W, generator=g).to(BF) if with_sem else None
    want = kr.patchify_ref(x, sem, 2)
    b, out = _flat(want.numel(), BF, cuda)
    ops.patchify(x.to(cuda), None if sem is None else sem.to(cuda), out, 2)
    torch.cuda.synchronize()
    kr.check_bits(b, _expect_flat(want), f"ld_patchify {shape} sem={with_sem}")


# ---- unpatchify + denoiser scaling + CFG -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scal", [(-0.7, 0.7, 1.0), (-0.35, 0.93, 6.5), (1.0, 0.0, 6.5)], ids=["scale1", "scale6.5", "cskip0"])
def test_unpatchify_cfg(cuda, scal):
    """Class A against eager fp32 torch with the last step as one fma (dit_video_concat.py:392-410, denoiser.py:25-41, guiders.py:75-79;
    the scalars as fp32 tensors, as the kernel receives them).  Against fully unfused torch: the rounding of scale * D apart (2^-24 of
    it, plus the final rounding landing on the neighbour), and equal at scale 1, where the product is exact and (c - u) + u returns
    the cond branch up to that one rounding."""
    from landiff_amd import ops
    T, C, H, W, p = 3, 4, 6, 10, 2
    g = torch.Generator().manual_seed(11)
    lin = torch.randn(2, T * (H // p) * (W // p), C * p * p, generator=g).to(BF)
    x = torch.randn(1, T, C, H, W, generator=g)
    want = kr.unpatchify_cfg_ref(lin, x, p, *scal)
    eager = kr.unpatchify_cfg_ref(lin, x, p, *scal, fused_last=False)
    n = want.numel()
    b, out = _flat(n, torch.float32, cuda, front=16)
    ops.unpatchify_cfg(lin.to(cuda), x.to(cuda), out.view(T, C, H, W), p, *scal)
    torch.cuda.synchronize()
    got = out.cpu().view(T, C, H, W)
    differ = (kr.bits(got) != kr.bits(eager)).sum().item()
    print(f"ld_unpatchify_cfg {scal}: {(kr.bits(got) != kr.bits(want)).sum().item()} of {n} elements differ from the stated form, {differ} from unfused eager torch")
    kr.check_bits(b, _expect_flat(want, front=16), f"ld_unpatchify_cfg {scal}")
    sd = (eager.double() - kr.unpatchify_cfg_ref(lin, x, p, scal[0], scal[1], 0.0, fused_last=False).double()).abs()      # |scale * D| (to a rounding)
    assert ((got.double() - eager.double()).abs() <= 2.0 ** -23 * (sd + eager.double().abs())).all(), "further than the product's rounding from eager torch"
    if scal[2] == 1.0:
        kr.check_bits(got, eager, "ld_unpatchify_cfg at scale 1 against unfused eager torch")


# ---- the sampler's elementwise update --------------------------------------------------------------------------------------
AXP_BIG = 16384 * 256 + 257        # one element more than grid_for's cap of 16384 workgroups covers in one trip, plus a ragged end


@pytest.fixture(scope="module")
def axp_data():
    g = torch.Generator().manual_seed(12)
    return tuple(torch.randn(AXP_BIG, generator=g) for _ in range(3))


@pytest.mark.parametrize("n", [1, 257, AXP_BIG])
def test_axpbypcz(cuda, axp_data, n):
    """Class A against fma(c, z, fma(b, y, a*x)) in the forms the sampler calls (sampling.py:613-644,750-783): x only, x + y, x + y + z,
    and in place on x.  n = 16384 * 256 + 257 is the one size that runs the grid-stride loop.  Against unfused eager torch: bit-equal
    in the x-only form, within a rounding of each fused product and of the two partial sums otherwise."""
    from landiff_amd import ops
    a, bb, c = 0.3, -1.7, 0.9
    x, y, z = (t[:n].contiguous() for t in axp_data)
    xd, yd, zd = x.to(cuda), y.to(cuda), z.to(cuda)
    for form, args, cpu_args in (("x", (), ()), ("x+y", (yd, bb), (y, bb)), ("x+y+z", (yd, bb, zd, c), (y, bb, z, c)),
                                 ("in place", (yd, bb, zd, c), (y, bb, z, c))):
        want = kr.axpbypcz_ref(x, a, *cpu_args)
        eager = kr.axpbypcz_ref(x, a, *cpu_args, fused=False)
        b, out = _flat(n, torch.float32, cuda, front=16)
        if form == "in place":
            out.copy_(xd)
            ops.axpbypcz(out, out, a, *args)
        else:
            ops.axpbypcz(out, xd, a, *args)
        torch.cuda.synchronize()
        got = out.cpu()
        print(f"ld_axpbypcz n={n} {form}: {(kr.bits(got) != kr.bits(eager)).sum().item()} of {n} elements differ from unfused eager torch")
        kr.check_bits(b, _expect_flat(want, front=16), f"ld_axpbypcz n={n} {form}")
        if form == "x":
            kr.check_bits(got, eager, "x only: eager torch")
        else:
            v1 = x.abs() * abs(a) + y.abs() * abs(bb)
            lim = (y.abs() * abs(bb) + z.abs() * abs(c)) * 2.0 ** -24 + 2.0 ** -23 * (v1 + got.abs())
            assert ((got - eager).abs() <= lim).all()


# ---- timestep embedding ------------------------------------------------------------------------------------------------------
_FULL, _TINY = PipelineConfig.full(), PipelineConfig.tiny()
TE_DIMS = sorted({_FULL.dit.hidden, _TINY.dit.hidden, _FULL.llm.freq_dim, _TINY.llm.freq_dim, 2, 7})     # dit.py:229 (temb [B, hidden]), llm.py:195 (freq_dim)
TE_T = [0.0, 1.0, 17.5, 500.0, 999.0]


@pytest.mark.parametrize("dim", TE_DIMS)
def test_timestep_embedding(cuda, dim):
    """Class B with an absolute bound, 2^-9 + |t| freq 2^-21 (kernel_ref.timestep_embedding_ref): cos || sin of t * exp(-ln(10000) j /
    half), util.py:207-233; the last column of an odd dim is zero.  B = 5 (every t) and B = 1; the CPU fp32 restatement is held to the
    same checker on the same data."""
    from landiff_amd import ops
    for ts in (TE_T, [17.5], [999.0]):
        t = torch.tensor(ts)
        ref, bound, cpu = kr.timestep_embedding_ref(t, dim)
        kr.check_abs_rounding(cpu, ref, bound, f"timestep embedding dim={dim} B={len(ts)}: CPU fp32")
        b, out = _flat(len(ts) * dim, BF, cuda)
        ops.timestep_embedding(t.to(cuda), out.view(len(ts), dim))
        torch.cuda.synchronize()
        got = out.cpu().view(len(ts), dim)
        kr.check_bits(b[len(ts) * dim:], kr.sentinels((TAIL,), BF), "behind the output")
        kr.check_abs_rounding(got, ref, bound, f"ld_timestep_embedding dim={dim} B={len(ts)}")
        if dim % 2:
            assert bool((kr.bits(got[:, -1]) == 0).all()), "the last column of an odd dim must be zero"


# ---- channels-last placement ---------------------------------------------------------------------------------------------------
def _place(cuda, x, mode, Cout, time_up, pads):
    from landiff_amd import ops
    Fn, Ti, Hi, Wi, Cin = x.shape
    want = kr.place_ref(x, mode, Cout, time_up)
    expect = kr.padded_expect(want, *pads)
    b = kr.sentinels((expect.numel() + TAIL,), BF, cuda)
    ops.place_cl(x.to(cuda), b.view(BF), Fn, Ti, Hi, Wi, Cin, Cout, mode=mode, time_up=time_up, tpad=pads[0], hpad=pads[1], wpad=pads[2])
    torch.cuda.synchronize()
    kr.check_bits(b, torch.cat([expect.reshape(-1), kr.sentinels((TAIL,), BF)]), f"ld_place_cl mode {mode} {tuple(x.shape)} -> C {Cout}, time_up={time_up}, pads {pads}")


@pytest.mark.parametrize("Cin,Cout,pads", [(16, 16, (0, 1, 1)), (16, 16, (2, 1, 1)), (3, 8, (2, 1, 1)), (8, 16, (2, 1, 1)), (16, 16, (0, 0, 0))],
                         ids=["c16_t0", "c16_t2", "c3to8", "c8to16", "nopads"])
def test_place_cl_copy(cuda, Cin, Cout, pads):
    """Class A, mode 0: the copy with F.pad's zero channels (cp_enc_dec.py:467-468) -- whole 16-byte chunks, the scalar tail of a partly
    filled chunk (3 -> 8), a whole zero chunk (8 -> 16).  Border cells and the tpad halo frames keep the sentinel."""
    g = torch.Generator().manual_seed(Cin + Cout)
    _place(cuda, torch.randn(2, 3, 5, 7, Cin, generator=g).to(BF), 0, Cout, False, pads)


@pytest.mark.parametrize("Ti,time_up", [(3, False), (1, True), (2, True), (3, True)])
def test_place_cl_upsample(cuda, Ti, time_up):
    """Class A, mode 1: F.interpolate(scale_factor=2, mode="nearest") applied exactly as Upsample3D.forward does (cp_enc_dec.py:605-627):
    2-d per frame without compress_time or with one frame; with it, 3-d, the first frame apart (and not doubled) when Ti is odd."""
    g = torch.Generator().manual_seed(Ti)
    _place(cuda, torch.randn(2, Ti, 5, 7, 16, generator=g).to(BF), 1, 16, time_up, (2, 1, 1))


def test_place_cl_pixel_shuffle(cuda):
    """Class A, mode 2: torch.nn.PixelShuffle(2) per frame (vq_gan_blocks.py:41-66), Cin 32 -> Cout 8."""
    g = torch.Generator().manual_seed(32)
    _place(cuda, torch.randn(2, 3, 5, 7, 32, generator=g).to(BF), 2, 8, False, (0, 1, 1))


@pytest.mark.parametrize("mode,Cin,Cout", [(1, 16, 8), (2, 16, 8), (0, 4, 12)], ids=["up_cin_ne_cout", "shuffle_cin_ne_4cout", "cout_not_8k"])
def test_place_cl_refusals(cuda, mode, Cin, Cout):
    from landiff_amd import ops
    from landiff_amd._lib import LandiffHipError
    x = torch.ones(1, 1, 2, 2, Cin, dtype=BF, device=cuda)
    b = kr.sentinels((4096,), BF, cuda)
    with pytest.raises(LandiffHipError):
        ops.place_cl(x, b.view(BF), 1, 1, 2, 2, Cin, Cout, mode=mode)
    torch.cuda.synchronize()
    assert bool(kr.is_sentinel(b).all())


# ---- [-1, 1] -> uint8 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_video", [True, False], ids=["video", "novideo"])
def test_to_uint8_every_finite_bf16(cuda, with_video):
    """Class A on every finite bf16 bit pattern and +-inf (which saturate): ((v + 1) / 2).clamp(0, 1) (dif_infer.py:37-49), then
    (. * 255).clamp(0, 255).to(uint8); the fp32 video [3][P] and the bytes [P][3] are both exact -- every step is one correctly rounded
    fp32 operation (the division by 2 is exact).  The values are the three used columns of a [P, 8] buffer (ldx = 8) whose other columns
    hold NaN sentinels."""
    from landiff_amd import ops
    v = torch.cat([kr.finite_bf16_patterns(), torch.tensor([float("inf"), float("-inf"), 0.0]).to(BF)])
    v = v[torch.randperm(v.numel(), generator=torch.Generator().manual_seed(13))].view(-1, 3)
    P = v.shape[0]
    assert P * 3 == 65283
    xb = kr.sentinels((P, 8), BF)
    xb[:, :3] = kr.bits(v)
    want8, want_video = kr.to_uint8_ref(v)
    b8, out8 = _flat(P * 3, torch.uint8, cuda)
    bv, video = _flat(3 * P, torch.float32, cuda)
    ops.to_uint8(xb.to(cuda).view(BF), out8, video if with_video else None, P)
    torch.cuda.synchronize()
    kr.check_bits(b8, _expect_flat(want8), "ld_to_uint8 bytes")
    if with_video:
        kr.check_bits(bv, _expect_flat(want_video), "ld_to_uint8 video")
    else:
        assert bool(kr.is_sentinel(bv).all())


# ---- latent -> the decoder's channels-last input ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mul", [1.0 / _FULL.vae.scale_factor, 1.0], ids=["inv_scale_factor", "one"])
@pytest.mark.parametrize("src_tchw", [False, True], ids=["cthw", "tchw"])
def test_latent_to_cl(cuda, src_tchw, mul):
    """Class A: samples.to(bf16), `1 / scale_factor * latent` as a bf16 multiply (dif_infer.py:251), channels-last with zero channels
    [C, Cpad) -- from both source layouts."""
    from landiff_amd import ops
    T, C, H, W, Cpad = 3, 16, 5, 7, 64
    g = torch.Generator().manual_seed(14)
    x = torch.randn((T, C, H, W) if src_tchw else (C, T, H, W), generator=g)
    want = kr.latent_to_cl_ref(x, T, C, H, W, Cpad, mul, src_tchw)
    assert not bool(want[..., C:].any())
    b, out = _flat(want.numel(), BF, cuda)
    ops.latent_to_cl(x.to(cuda), out, T, C, H, W, Cpad, mul, src_tchw)
    torch.cuda.synchronize()
    kr.check_bits(b, _expect_flat(want), f"ld_latent_to_cl tchw={src_tchw} mul={mul}")
