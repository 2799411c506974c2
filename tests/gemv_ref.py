"""The reference, the case table and the checker of the decode GEMV's direct tests (ld_gemv, landiff_amd/csrc/ld_llm_gemv.hip):
tests/test_gpu_gemv_routes.py runs the cases on the GPU, tests/test_gemv_ref_host.py runs the reference against a plain fp32
restatement on the CPU (must pass) and against deliberately wrong outputs (must fail), and checks the route column of the table.

Pure torch (any device) apart from `route`, which asks the library for ld_gemv's own dispatch plan (host logic, no GPU needed).
The checkers, sentinels and the bf16 ulp are those of tests/kernel_ref.py and tests/test_gpu_gemm_routes.py.
"""
import ctypes
import functools
import zlib

import torch
import torch.nn.functional as F

from kernel_ref import BF, bf, bits, check_bits, check_chain, check_f32, round_bf, sentinels
from test_gpu_gemm_routes import ACT64, _check_sentinels, _ulp

STREAM, REG = 0, 1                       # ld_gemv_route's return values
ACT32 = {"silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh")}


# ------------------------------------------------------------------------------------------------------------------------------
# the plan
# ------------------------------------------------------------------------------------------------------------------------------
def route(B, N, K, *, x_f32=False, w_f32=False, out_f32=False, gated=False, normed=False, in_act=False):
    """ld_gemv_route -> (kind or negative code, J, R, U)."""
    from landiff_amd import _lib
    J, R, U = (ctypes.c_int32(-1) for _ in range(3))
    rc = _lib.load().ld_gemv_route(B, N, K, int(x_f32), int(w_f32), int(out_f32), int(gated), int(normed), int(in_act),
                                   ctypes.byref(J), ctypes.byref(R), ctypes.byref(U))
    return rc, J.value, R.value, U.value


def chain_length(plan, K):
    """n_add of gemv_reference: the longest chain of fp32 additions behind one output of the planned kernel.
    Register kernel: a thread owns J chunks of 8 elements = 4 J dot2 steps, each an add of a two-product sum to the accumulator
    (counted as 8 J element additions), then the 6 steps of the wave butterfly and the 3 additions of the four waves' totals.
    Streaming kernel: a lane takes U chunks per trip over K, ntrip = ceil(K / 8 / (64 U)) trips, one fma per element into the same
    accumulator (8 U ntrip), then the 6 butterfly steps."""
    kind, J, R, U = plan
    if kind == REG:
        return 8 * J + 6 + 3
    nchunk = K // 8
    return 8 * U * ((nchunk + 64 * U - 1) // (64 * U)) + 6


# ------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------
def staged_x(x, w_f32, in_act, norm_w, eps):
    """The activations as the kernels feed them to the dot product -> (xn float64, amb float64).
    fp32 weights: x as it is.  bf16 weights: bf16(x) (the staging rounds an fp32 x), bf16(act(x)) with in_act,
    bf16(x * rsqrt(mean x^2 + eps) * g) with norm_w (transformer_blocks.py:22-40).
    amb: the kernel evaluates the activation / the norm in fp32, and its bf16 rounding can fall to the other side only where a
    rounding midpoint lies within that evaluation's error of the float64 value: 2^-20 (|v| + |act(v)|) for an activation (the
    constant of test_gpu_gemm_routes._reference), 2^-20 |v| for the norm (an fp32 sum of squares, a division, rsqrt, two products).
    amb is one bf16 ulp there and 0 everywhere else -- carrying an ulp for EVERY element through a K-term sum would add up to tens of
    output ulps."""
    v = x.double()
    zero = torch.zeros_like(v)
    if w_f32:
        assert in_act is None and norm_w is None, "fp32 weights with an activation or a norm is not a shipped form"
        return v, zero
    assert not (in_act and norm_w is not None), "in_act with norm_w is refused by ld_gemv"
    if in_act:
        fv = ACT64[in_act](v)
        e = 2.0 ** -20 * (v.abs() + fv.abs())
        v = fv
    elif norm_w is not None:
        v = v * torch.rsqrt(v.square().mean(-1, keepdim=True) + eps) * norm_w.double()
        e = 2.0 ** -20 * v.abs()
    else:
        return bf(v), zero                                   # one correct rounding of exact inputs on both sides
    amb = bf(v - e) != bf(v + e)
    return bf(v), torch.where(amb, _ulp(v.abs() + e), zero)


def gemv_reference(x, w, *, w2=None, bias=None, resid=None, in_act=None, act=None, norm_w=None, eps=0.0, out_f32=False, n_add,
                   exact=False):
    """ld_gemv in float64, rounded where the kernels round (ld_gemv_kernel's and ld_gemv_reg_kernel's epilogues, the same chain:
    + bias, round (bf16 weights), act and round, gated: round(v * round(acc2)), resid + v rounded unless out_f32)
    -> (value float64 [B, N], bound float64 [B, N]).

    The bound is derived, not measured.  The dot product of the staged activations xn carries
      * sum_k amb_k |w_k|: the activations whose bf16 rounding is ambiguous (staged_x); zero for most rows;
      * 2 n_add 2^-24 sum_k |xn_k w_k|: n_add fp32 additions in the longest chain (chain_length, from the plan), each rounding a
        partial sum that is at most sum |xn w| in size to 2^-24 of it; bf16 products are exact in fp32; the factor 2 covers dot2's
        internal addition of its two products before the accumulator is added;
    and every later step adds what kernel_ref.round_bf / test_gpu_gemm_routes._reference add: one bf16 ulp per rounding point, the
    earlier error through the activation's slope and the gate factor, 2^-20 (|v| + |act(v)|) for the fp32 activation.
    exact: asserts that every rounded value is a bf16 number already (operands of `operands(case, exact=True)`); the bound is 0.
    fp32 weights: the float64 value only (class B: check_f32 against torch's fp32 on the CPU), bound None."""
    w_f32 = w.dtype == torch.float32
    xn, amb = staged_x(x, w_f32, in_act, norm_w, eps)
    wd = w.double()
    acc = xn @ wd.t()
    if w_f32:
        assert w2 is None and act is None
        v = acc + (bias.double() if bias is not None else 0.0)
        return (v + resid.double() if resid is not None else v), None
    if exact:
        assert in_act is None and act is None and norm_w is None and w2 is None, "activations, norms and gates are checked with random operands"
        err = torch.zeros_like(acc)
    else:
        err = amb @ wd.abs().t() + (xn.abs() @ wd.abs().t()) * (2 * n_add * 2.0 ** -24)

    def rnd(v, err, what):
        if exact:
            assert torch.equal(v, bf(v)), f"premise: {what} is not exact in bf16"
            return v, err
        return round_bf(v, err)

    v = acc + bias.double() if bias is not None else acc
    v, err = rnd(v, err, "the Linear output")
    if act:
        fv = ACT64[act](v)
        slope = torch.maximum((ACT64[act](v + err) - fv).abs(), (ACT64[act](v - err) - fv).abs())
        v, err = rnd(fv, slope + 2.0 ** -20 * (v.abs() + fv.abs()) + 2.0 ** -120, "the activation")
    if w2 is not None:
        w2d = w2.double()
        g, eg = rnd(xn @ w2d.t(), amb @ w2d.abs().t() + (xn.abs() @ w2d.abs().t()) * (2 * n_add * 2.0 ** -24), "W2 x")
        v, err = rnd(v * g, err * g.abs() + v.abs() * eg + err * eg, "the gate product")
    if resid is not None:
        v = resid.double() + v
        if out_f32:
            if exact:
                assert torch.equal(v, v.float().double()), "premise: the fp32 sum is not exact"
            else:
                err = err + 2.0 ** -24 * (v.abs() + err)      # one fp32 rounding, not a bf16 one
                v = v.float().double()
        else:
            v, err = rnd(v, err, "resid + y")
    return v, err


def gemv_cpu32(x, w, *, w2=None, bias=None, resid=None, in_act=None, act=None, norm_w=None, eps=0.0, out_f32=False, k_mult=None,
               drop=None):
    """The kernels' chain restated in plain torch fp32 on the CPU (eager ops, torch's own summation order) -> out's dtype [B, N].
    k_mult (fp32 [K]) and drop are the host test's wrong kernels: every staged activation k counted k_mult[k] times; drop names
    a rounding point left out ("linear": the Linear output before act, "acc2": W2 x before the gate product) or put in
    ("resid": the residual sum rounded although out_f32)."""
    rb = lambda t: t.to(BF).float()
    xf = x.float()
    if w.dtype == torch.float32:
        y = xf @ w.t()
        if bias is not None:
            y = y + bias.float()
        return y + resid if resid is not None else y
    if in_act:
        xf = ACT32[in_act](xf)
    elif norm_w is not None:
        xf = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * norm_w
    xf = rb(xf)
    if k_mult is not None:
        xf = xf * k_mult
    y = xf @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if drop != "linear":
        y = rb(y)
    if act:
        y = rb(ACT32[act](y))
    if w2 is not None:
        y2 = xf @ w2.float().t()
        y = rb(y * (y2 if drop == "acc2" else rb(y2)))
    if resid is not None:
        y = resid.float() + y
        if not out_f32 or drop == "resid":
            y = rb(y)
    return y if out_f32 else y.to(BF)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """form: a set of "bias", "norm", "gated" (act gelu_tanh on W x, times W2 x: LlamaMLP2), "resid", "inplace" (out is resid),
    "silu" (output activation), "in_silu", "xf32" (fp32 x on bf16 weights), "f32" (fp32 weights, x, out), "f32out" (bf16 x / W,
    fp32 out and residual).  plan: what ld_gemv_route must answer, (kind, J, R, U)."""

    def __init__(self, id, B, N, K, form, plan, edge=""):
        self.id, self.B, self.N, self.K, self.form, self.plan, self.edge = id, B, N, K, frozenset(form.split()), plan, edge
        assert self.form <= {"bias", "norm", "gated", "resid", "inplace", "silu", "in_silu", "xf32", "f32", "f32out"}, form

    has = lambda self, f: f in self.form
    w_f32 = property(lambda self: "f32" in self.form)
    x_f32 = property(lambda self: "f32" in self.form or "xf32" in self.form)
    out_f32 = property(lambda self: "f32" in self.form or "f32out" in self.form)
    in_act = property(lambda self: "silu" if "in_silu" in self.form else None)
    act = property(lambda self: "gelu_tanh" if "gated" in self.form else "silu" if "silu" in self.form else None)
    has_exact = property(lambda self: not (self.form & {"norm", "gated", "silu", "in_silu"}))       # no act, no norm: also run exact
    seed = property(lambda self: zlib.crc32(self.id.encode()))

    def route(self):
        return route(self.B, self.N, self.K, x_f32=self.x_f32, w_f32=self.w_f32, out_f32=self.out_f32, gated=self.has("gated"),
                     normed=self.has("norm"), in_act=self.in_act is not None)

    def key(self):
        """The instantiation (and the staging / epilogue branches the issue counts with it) a case exercises."""
        return self.plan + (self.has("gated"), self.has("norm"), min(self.B, 3), self.w_f32)

    def __repr__(self):
        return self.id


S14, S24, S81 = (STREAM, 0, 1, 4), (STREAM, 0, 2, 4), (STREAM, 0, 8, 1)
reg = lambda J, R: (REG, J, R, 0)

# The smallest shape at which each edge exists (the largest weight matrix: 34 MB).
TABLE = [
    Case("r_grid", 2, 3081, 64, "bias", reg(1, 4), "771 batches > 768: two trips, the last workgroup has one batch"),
    Case("r_onechunk", 1, 5, 8, "norm", reg(1, 4), "one chunk, waves 1-3 empty, N = R + 1"),
    Case("r_255", 4, 7, 2040, "gated norm", reg(1, 4), "255 chunks, V = 32 partial sums"),
    Case("r_j1_full", 3, 9, 2048, "resid inplace", reg(1, 4), "B = 3 epilogue indexing"),
    Case("r_j2_first", 2, 6, 2056, "norm bias", reg(2, 4), "chunk 256 on thread 0 only"),
    Case("r_j2_gated", 4, 5, 4096, "gated resid", reg(2, 2), "gated without norm"),
    Case("r_f32out", 3, 4, 4096, "f32out resid", reg(2, 4), "raw 32-bit residual, sum not rounded"),
    Case("r_j6_first", 2, 3, 4104, "norm", reg(6, 2), "513 chunks"),
    Case("r_j6_full", 1, 2, 12288, "bias silu", reg(6, 2), "last register shape"),
    Case("r_w2", 2, 33, 11008, "resid inplace", reg(6, 2), "the decoder's w2: j = 5 holds 96 chunks"),
    Case("s_past_j6", 2, 3, 12296, "resid", S14, "1537 chunks: the 7th trip holds one"),
    Case("s_norm", 3, 5, 4104, "norm", S14, "fused norm in the staging, 3 trips"),
    Case("s_gated_norm", 4, 3, 4104, "gated norm", S14, "gated staging path"),
    Case("s_gated_loop", 1, 2050, 4104, "gated", S14, "2050 groups over 2048 waves"),
    Case("s_r2", 2, 4098, 520, "in_silu bias", S24, "65 chunks; 2049 groups: one wave takes two"),
    Case("s_r8_tail", 4, 4099, 512, "in_silu bias", S81, "N % 8 = 3"),
    Case("s_r8_onechunk", 1, 4096, 8, "in_silu", S81, "lanes 1-63 idle"),
    Case("s_xf32", 2, 7, 1920, "xf32 bias", S14, "the DiT temb -> te0 form"),
    Case("s_two_trips", 2, 9, 2056, "in_silu bias resid", S14, "epilogue operands prefetched with the last trip"),
    Case("f_head", 2, 2055, 2048, "f32", S14, "the LM head"),
    Case("f_small", 4, 3, 8, "f32 bias resid", S14, ""),
    Case("f_loop", 1, 2049, 2056, "f32", S14, "2 trips, 2049 groups"),
]


def _coverage_cases():
    """One tiny case for every instantiation the default dispatch reaches and TABLE does not: every (kernel, J, R, U, gated, norm)
    x B in {1, 2, 3-4} (the register J = 6 forms: B <= 2).  N = R + 1 (a second, partial batch) or just past 4096 where the plan
    asks for many rows; K the first chunk count of each J / the first past the register forms."""
    have = {c.key() for c in TABLE}
    out = []

    def add(id, B, N, K, form, plan):
        c = Case(id, B, N, K, form, plan, "coverage")
        if c.key() not in have:
            have.add(c.key())
            out.append(c)

    for Bc in (1, 2, 3):
        b34 = lambda i: Bc if Bc < 3 else 3 + i % 2          # the 3-4 class: B = 3 and B = 4 in turn
        for J, K in ((1, 72), (2, 2056)):
            for gated in (False, True):
                for norm in (False, True):
                    R, B = (2 if (J == 2 and gated) else 4), b34(J + gated + norm)
                    form = ("gated" if gated else "bias resid") + (" norm" if norm else "")
                    add(f"c_reg_j{J}{'g' if gated else ''}{'n' if norm else ''}_b{B}", B, R + 1, K, form, reg(J, R))
        if Bc <= 2:
            for norm in (False, True):
                add(f"c_reg_j6{'n' if norm else ''}_b{Bc}", Bc, 3, 4104, "norm" if norm else "bias resid", reg(6, 2))
        add(f"c_s14_b{b34(0)}", b34(0), 5, 12296, "bias resid", S14)
        add(f"c_s14n_b{b34(1)}", b34(1), 3, 12296 if Bc <= 2 else 4104, "norm", S14)
        add(f"c_s14g_b{b34(0)}", b34(0), 3, 4104, "gated", S14)
        add(f"c_s14gn_b{b34(1)}", b34(1), 3, 4104, "gated norm", S14)
        add(f"c_s24_b{b34(0)}", b34(0), 4097, 520, "in_silu bias", S24)
        add(f"c_s81_b{b34(1)}", b34(1), 4097, 64, "in_silu bias", S81)
    add("c_s24n_b3", 3, 4097, 4104, "norm", S24)
    return out


COVERAGE = _coverage_cases()
CASES = TABLE + COVERAGE

# Reached by the default dispatch and not run: the streaming kernel with two rows per wave behind the fused norm for B <= 2 needs
# N >= 4096 at K > 12288, a 100 MB matrix; the staging (where the norm is) runs before anything that depends on R, and the same
# instantiations run without the norm (s_r2, c_s24_b1) and with it at B = 3 (c_s24n_b3).
NOT_COVERED = {S24 + (False, True, 1, False), S24 + (False, True, 2, False)}


@functools.lru_cache(maxsize=2)
def operands(case, exact):
    """The operands of a case, made once on the CPU (placed() hands them out): xbuf [B, K + 8] whose last 8 columns hold NaN, w
    (row-dependent structure in column 0, as tests/test_gpu_gemv.py: catches row mix-ups), w2, bias, rbuf [B, N + 5], norm_w.
    exact: ternary x and W at density sqrt(8 / K), small-integer bias and residual (test_gpu_gemm_routes._operands): every fp32
    sum and every rounded value is exact."""
    B, N, K = case.B, case.N, case.K
    g = torch.Generator().manual_seed(case.seed + int(exact))
    xdt, wdt, odt = (torch.float32 if f else BF for f in (case.x_f32, case.w_f32, case.out_f32))
    n = torch.arange(N)
    if exact:
        dens = (8.0 / K) ** 0.5
        tern = lambda r, c: (torch.randint(-1, 2, (r, c), generator=g) * (torch.rand(r, c, generator=g) < dens)).float()
        xv, w = tern(B, K), tern(N, K)
        w[:, 0] = (n % 3 - 1).float()
    else:
        xv, w = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
        w = w.to(wdt).float()
        w[:, 0] += (n % 7).float() * 0.05
    xbuf = torch.full((B, K + 8), float("nan"), dtype=xdt)
    xbuf[:, :K] = xv.to(xdt)
    o = dict(xbuf=xbuf, w=w.to(wdt).contiguous(), w2=None, bias=None, rbuf=None, norm_w=None)
    if case.has("gated"):
        o["w2"] = (torch.randn(N, K, generator=g) * K ** -0.5).to(wdt)
    if case.has("norm"):
        o["norm_w"] = 1.0 + 0.1 * torch.randn(K, generator=g)
    if case.has("bias"):
        o["bias"] = (torch.randint(-4, 5, (N,), generator=g).float() if exact else torch.randn(N, generator=g) * 0.5).to(BF)
    if case.has("resid"):
        rbuf = torch.zeros(B, N + 5, dtype=odt)
        rbuf[:, :N] = (torch.randint(-8, 9, (B, N), generator=g).float() if exact else torch.randn(B, N, generator=g)).to(odt)
        o["rbuf"] = rbuf
    return o


def placed(case, exact, device="cpu"):
    """A case's operands on `device` as the kernel gets them: x a [B, K] view of the [B, K + 8] buffer (ldx = K + 8; a chunk read
    past K reads NaN and poisons the sum), resid a [B, N] view with its own row stride N + 5 (!= ldo), the rest contiguous."""
    o = {k: (v.to(device) if v is not None else None) for k, v in operands(case, exact).items()}
    o["x"] = o.pop("xbuf")[:, :case.K]
    rbuf = o.pop("rbuf")
    o["resid"] = rbuf[:, :case.N] if rbuf is not None else None
    assert o["x"].stride(0) == case.K + 8 and (rbuf is None or o["resid"].stride(0) == case.N + 5)
    return o


def call_kwargs(case, o):
    """The keyword arguments of ops.gemv / gemv_reference / gemv_cpu32 that a case's operands make (eps under each one's own name)."""
    kw = dict(w2=o["w2"], bias=o["bias"], resid=o["resid"], in_act=case.in_act, act=case.act, norm_w=o["norm_w"])
    return kw, (1e-5 if case.has("norm") else 0.0)


def out_buffer(case, device="cpu"):
    """out as a [B, N] view in a [B + 2, ldo] buffer of sentinels, ldo = N + 3 -> (buffer bits, out view)."""
    dt = torch.float32 if case.out_f32 else BF
    b = sentinels((case.B + 2, case.N + 3), dt, device)
    return b, b.view(dt)[:case.B, :case.N]


def reference(case, o, exact):
    """(value, bound, torch32) of a case on the device of its operands: gemv_reference with the chain length of the case's plan;
    fp32 weights with random operands: bound None and torch's fp32 evaluation on the CPU for check_f32."""
    kw, eps = call_kwargs(case, o)
    ref, bound = gemv_reference(o["x"], o["w"], eps=eps, out_f32=case.out_f32, n_add=chain_length(case.plan, case.K), exact=exact, **kw)
    t32 = None
    if case.w_f32 and not exact:
        cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in o.items()}
        t32 = gemv_cpu32(cpu["x"], cpu["w"], bias=cpu["bias"], resid=cpu["resid"], out_f32=True)
    return ref, bound, t32


def check_case(case, buf, ref, bound, t32, exact, what):
    """The whole check of one run: buf is out_buffer's sentinel buffer after the kernel.  exact: check_bits on the WHOLE buffer
    (the expected one holds the sentinel outside [0, B) x [0, N)); random: check_chain (bf16 weights) or check_f32 (fp32 weights) on
    the output, then every sentinel outside it intact.  Returns what the checker returns."""
    B, N = case.B, case.N
    dt = torch.float32 if case.out_f32 else BF
    if exact:
        want = sentinels(tuple(buf.shape), dt)
        want[:B, :N] = bits(ref.to(dt).cpu())
        check_bits(buf, want, what)
        return 0.0, 1.0
    out = buf.view(dt)[:B, :N]
    res = check_f32(out.cpu(), ref.cpu(), t32, what) if t32 is not None else check_chain(out, ref, bound, what)
    _check_sentinels(buf, B, N)
    return res
