"""Thin tensor-level wrappers over the C ABI (include/landiff_hip.h).

torch is used only for device memory and the current HIP stream; all arithmetic happens in
liblandiff_hip.so.  Every wrapper raises if its tensors are not on a GPU.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import Epilogue, check

ACT = {None: 0, "none": 0, "gelu_tanh": 1, "gelu_erf": 2, "silu": 3, "tanh": 4}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: torch.Tensor | None):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.LandiffHipError("landiff_amd ops need GPU tensors (no CPU fallback)")
    return ctypes.c_void_p(t.data_ptr())


def _bf16(t: torch.Tensor, name: str):
    if t.dtype != torch.bfloat16:
        raise TypeError(f"{name} must be bfloat16, got {t.dtype}")


def make_epilogue(
    *,
    bias=None,
    act=None,
    mul=None,
    resid=None,
    gate=None,
    gate_bstride=0,
    gate_off_img=0,
    gate_off_txt=0,
    rows_per_batch=0,
    text_len=0,
    add2=None,
    out_f32=False,
) -> Epilogue:
    e = Epilogue()
    e.bias = _ptr(bias)
    e.act = ACT[act]
    e.mul = _ptr(mul)
    e.ldmul = mul.stride(-2) if mul is not None else 0
    e.resid = _ptr(resid)
    e.ldr = resid.stride(-2) if resid is not None else 0
    e.resid_f32 = int(resid is not None and resid.dtype == torch.float32)
    e.gate = _ptr(gate)
    e.gate_bstride = gate_bstride
    e.gate_off_img = gate_off_img
    e.gate_off_txt = gate_off_txt
    e.rows_per_batch = rows_per_batch
    e.text_len = text_len
    e.add2 = _ptr(add2)
    e.ldadd = add2.stride(-2) if add2 is not None else 0
    e.out_f32 = int(out_f32)
    return e


def gemm(a: torch.Tensor, w: torch.Tensor, out: torch.Tensor | None = None, **epi) -> torch.Tensor:
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T).  a may have a row stride (last dim contiguous)."""
    _bf16(a, "a"); _bf16(w, "w")
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.is_contiguous()
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out_f32 = bool(epi.get("out_f32", False))
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.stride(1) == 1 and out.shape == (M, N)
    assert (out.dtype == torch.float32) == out_f32
    e = make_epilogue(**epi)
    lib = _lib.load()
    check(lib.ld_gemm_bf16(_ptr(a), a.stride(0), _ptr(w), _ptr(out), out.stride(0), M, N, K,
                           ctypes.byref(e), _stream()), "ld_gemm_bf16")
    return out


def quantize_fp8(x: torch.Tensor, q: torch.Tensor | None = None, scale: torch.Tensor | None = None):
    """Row-wise dynamic e4m3 quantisation: x bf16 [M,K] -> (q uint8 [M,K], scale fp32 [M]); x ~= q * scale[:, None]."""
    _bf16(x, "x")
    M, K = x.shape
    assert x.stride(1) == 1
    if q is None:
        q = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    if scale is None:
        scale = torch.empty(M, device=x.device, dtype=torch.float32)
    assert q.dtype == torch.uint8 and q.shape == (M, K) and q.stride(1) == 1 and scale.dtype == torch.float32 and scale.is_contiguous()
    check(_lib.load().ld_quantize_fp8(_ptr(x), x.stride(0), _ptr(q), q.stride(0), _ptr(scale), M, K, _stream()), "ld_quantize_fp8")
    return q, scale


def gemm_fp8(a8: torch.Tensor, scale_a: torch.Tensor, w8: torch.Tensor, scale_w: torch.Tensor,
             out: torch.Tensor | None = None, **epi) -> torch.Tensor:
    """out[M,N] = epilogue((a8 * scale_a[:,None]) @ (w8 * scale_w[:,None])^T), e4m3 operands as uint8 tensors."""
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and a8.stride(1) == 1 and w8.is_contiguous()
    M, K = a8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and scale_a.shape == (M,) and scale_w.shape == (N,)
    assert scale_a.dtype == torch.float32 and scale_w.dtype == torch.float32 and scale_a.is_contiguous() and scale_w.is_contiguous()
    out_f32 = bool(epi.get("out_f32", False))
    if out is None:
        out = torch.empty((M, N), device=a8.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.stride(1) == 1 and out.shape == (M, N) and (out.dtype == torch.float32) == out_f32
    e = make_epilogue(**epi)
    check(_lib.load().ld_gemm_fp8(_ptr(a8), a8.stride(0), _ptr(scale_a), _ptr(w8), _ptr(scale_w), _ptr(out), out.stride(0),
                                  M, N, K, ctypes.byref(e), _stream()), "ld_gemm_fp8")
    return out


def quantize_mxfp8(x: torch.Tensor, q: torch.Tensor | None = None, scales: torch.Tensor | None = None):
    """MXFP8 quantisation: x bf16 [M,K] -> (q uint8 [M,K] e4m3 codes, scales uint8 [K/128, M, 4] E8M0 bytes, K-tile-major)."""
    _bf16(x, "x")
    M, K = x.shape
    assert x.stride(1) == 1 and K % 128 == 0
    if q is None:
        q = torch.empty(M, K, device=x.device, dtype=torch.uint8)
    if scales is None:
        scales = torch.empty(K // 128, M, 4, device=x.device, dtype=torch.uint8)
    assert q.dtype == torch.uint8 and q.shape == (M, K) and q.stride(1) == 1
    assert scales.dtype == torch.uint8 and tuple(scales.shape) == (K // 128, M, 4) and scales.is_contiguous()
    check(_lib.load().ld_quantize_mxfp8(_ptr(x), x.stride(0), _ptr(q), q.stride(0), _ptr(scales), M, M, K,
                                        _stream()), "ld_quantize_mxfp8")
    return q, scales


def gemm_mxfp8(a8: torch.Tensor, sa: torch.Tensor, w8: torch.Tensor, sw: torch.Tensor, out: torch.Tensor | None = None,
               out_scales: torch.Tensor | None = None, **epi) -> torch.Tensor:
    """out[M,N] = epilogue(dequant(a8, sa) @ dequant(w8, sw)^T) with the MX block scales applied inside the MFMA.
    out_scales (uint8 [N/128, M, 4]): the output is MXFP8 too (out uint8 [M,N]); bias + act="gelu_tanh" only."""
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and a8.stride(1) == 1 and w8.is_contiguous()
    M, K = a8.shape
    N = w8.shape[0]
    assert w8.shape[1] == K and tuple(sa.shape) == (K // 128, M, 4) and tuple(sw.shape) == (K // 128, N, 4)
    assert sa.dtype == torch.uint8 and sw.dtype == torch.uint8 and sa.is_contiguous() and sw.is_contiguous()
    out_f32 = bool(epi.get("out_f32", False))
    if out_scales is not None:
        assert out is not None and out.dtype == torch.uint8 and out_scales.dtype == torch.uint8
        assert tuple(out_scales.shape) == (N // 128, M, 4) and out_scales.is_contiguous()
    elif out is None:
        out = torch.empty((M, N), device=a8.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.stride(1) == 1 and out.shape == (M, N)
    assert out_scales is not None or (out.dtype == torch.float32) == out_f32
    e = make_epilogue(**epi)
    check(_lib.load().ld_gemm_mxfp8(_ptr(a8), a8.stride(0), _ptr(sa), _ptr(w8), _ptr(sw), _ptr(out), out.stride(0),
                                    _ptr(out_scales), M if out_scales is not None else 0,
                                    M, N, K, ctypes.byref(e), _stream()), "ld_gemm_mxfp8")
    return out


def conv_cl(x_padded: torch.Tensor, w: torch.Tensor, T: int, H: int, W: int,
            out: torch.Tensor | None = None, gn_partials: bool = False, **epi):
    """Channels-last conv.  x_padded [T+kT-1, H+kH-1, W+kW-1, Cin]; w [Cout, kT, kH, kW, Cin].
    gn_partials=True: returns (out, partials) -- the epilogue also leaves the GroupNorm partial sums of the bf16 output
    (fp32 [ceil(M / 64)][Cout / 4][2]) for groupnorm_stats_from_conv, instead of a second read of the activation."""
    _bf16(x_padded, "x_padded"); _bf16(w, "w")
    assert x_padded.is_contiguous() and w.is_contiguous() and w.dim() == 5
    Cout, kT, kH, kW, Cin = w.shape
    assert tuple(x_padded.shape) == (T + kT - 1, H + kH - 1, W + kW - 1, Cin), (x_padded.shape, w.shape, T, H, W)
    out_f32 = bool(epi.get("out_f32", False))
    if out is None:
        out = torch.empty((T * H * W, Cout), device=x_padded.device,
                          dtype=torch.float32 if out_f32 else torch.bfloat16)
    assert out.stride(-1) == 1
    e = make_epilogue(**epi)
    lib = _lib.load()
    if gn_partials:
        part = torch.empty(int(lib.ld_conv_gn_partials_size(T * H * W, Cout)), device=x_padded.device, dtype=torch.float32)
        check(lib.ld_conv_cl_bf16_gn(_ptr(x_padded), _ptr(w), _ptr(out), out.stride(-2), T, H, W, Cin, Cout,
                                     kT, kH, kW, ctypes.byref(e), _ptr(part), _stream()), "ld_conv_cl_bf16_gn")
        return out, part
    check(lib.ld_conv_cl_bf16(_ptr(x_padded), _ptr(w), _ptr(out), out.stride(-2), T, H, W, Cin, Cout,
                              kT, kH, kW, ctypes.byref(e), _stream()), "ld_conv_cl_bf16")
    return out


ATTN_KEY_TILE = 64                 # keys per tile of the attention kernels (kt_min / kt_max granularity)
ATTN_PIPELINED_MIN_TILES = 6       # unmasked problems of at least this many key tiles take the pipelined kernels (the library's
                                   # constant of that name: tests/test_attn_route_host.py finds it through attn_route)
ATTN_FORMS = {"default": 0, "exact": 1, "window": 2}


def attn_route(B: int, H: int, Nq: int, Nk: int, Npad: int, masked: bool = False, form: str = "default") -> int:
    """ld_attn_route: the kernel family an attn_fwd (form "default" / "exact") or attn_fwd_window ("window") launch of these shapes
    would run under the current LD_ATTN_* knobs -- 0 plain, 1 q64, 2 q64 exact, 3 q64 window, 4 p16, 5 q128, 6 pipe2 -- or
    LandiffHipError with the launch's own refusal.  Host only: nothing is launched, no GPU needed."""
    lib = _lib.load()
    rc = lib.ld_attn_route(B, H, Nq, Nk, Npad, int(bool(masked)), ATTN_FORMS[form])
    if rc < 0:
        check(rc, "ld_attn_route")
    return rc


def attn_mask_tables(fid_q, fid_k, Npad: int, device=None):
    """The four int32 arrays of ld_attn_fwd_bf16's label mask (allowed(q, kv) <=> fid_k[kv] <= fid_q[q]) from the labels of the
    real rows: (fid_q [Npad] padded with 0, fid_k [Npad] padded with INT32_MAX so that no query sees a padding key,
    kt_min, kt_max [Npad / 64] = the smallest / largest fid_k of each 64-key tile), as tensors on `device`."""
    fid_q, fid_k = np.asarray(fid_q), np.asarray(fid_k)
    assert fid_q.ndim == 1 and fid_k.ndim == 1 and Npad % 128 == 0 and len(fid_q) <= Npad and len(fid_k) <= Npad
    fq = np.zeros(Npad, np.int32); fq[:len(fid_q)] = fid_q
    fk = np.full(Npad, np.iinfo(np.int32).max, np.int32); fk[:len(fid_k)] = fid_k
    kt = fk.reshape(-1, ATTN_KEY_TILE)
    return tuple(torch.from_numpy(x).to(device) for x in (fq, fk, kt.min(1).copy(), kt.max(1).copy()))


def attn_fwd(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, Nq: int, Nk: int,
             scale: float, fid_q=None, fid_k=None, kt_min=None, kt_max=None, q_row0: int = 0, exact: bool = False) -> torch.Tensor:
    """q,k [B,H,Npad,64]; vt [B,H,64,Npad]; out [B,N,H*64] (bf16).  Optional frame mask arrays (int32; attn_mask_tables).
    q_row0: the Nq query rows start at row q_row0 of q / fid_q / out (pointer offsets only; Npad must cover
    q_row0 + Nq rounded up to 128).  exact: ld_attn_fwd_bf16_exact -- the two-pass safe softmax at a fixed ~1.55 x, for logit
    ranges beyond the window of the default launch's fast pass.
    q_row0 != 0 needs the label mask or fewer than 6 key tiles, i.e. the plain kernel, which reads Q rows only up to Nq rounded
    up to 128 (the assert below keeps those inside this head's rows).  The pipelined kernels of unmasked problems of >= 6 key
    tiles work in 256-row query blocks and clamp the Q row to Npad - 1 counted from the OFFSET pointer, so a live block could
    read up to 128 rows past this head's rows -- past the end of the tensor for the last head: ValueError, before any launch."""
    if q_row0 and fid_k is None and (Nk + ATTN_KEY_TILE - 1) // ATTN_KEY_TILE >= ATTN_PIPELINED_MIN_TILES:
        raise ValueError(f"attn_fwd: q_row0={q_row0} without a label mask on {Nk} keys (>= {ATTN_PIPELINED_MIN_TILES} key tiles) "
                         "would run a pipelined kernel that reads Q rows past the offset block")
    _bf16(q, "q"); _bf16(k, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    B, H, Npad, D = q.shape
    assert D == 64 and k.shape == q.shape and tuple(vt.shape) == (B, H, 64, Npad)
    assert q.is_contiguous() and k.is_contiguous() and vt.is_contiguous() and out.stride(-1) == 1
    assert out.shape[0] == B and out.shape[2] == H * 64
    lib = _lib.load()
    qp, op, fqp = _ptr(q), _ptr(out), _ptr(fid_q)
    if q_row0:
        assert B == 1 and q_row0 % 2 == 0 and q_row0 + (Nq + 127) // 128 * 128 <= Npad
        qp = ctypes.c_void_p(qp.value + q_row0 * 64 * 2)
        op = ctypes.c_void_p(op.value + q_row0 * out.stride(1) * 2)
        fqp = ctypes.c_void_p(fqp.value + q_row0 * 4) if fqp is not None else None
    fn = lib.ld_attn_fwd_bf16_exact if exact else lib.ld_attn_fwd_bf16
    check(fn(qp, _ptr(k), _ptr(vt), op, B, H, Nq, Nk, Npad, out.stride(0), out.stride(1), float(scale),
             fqp, _ptr(fid_k), _ptr(kt_min), _ptr(kt_max), _stream()),
          "ld_attn_fwd_bf16_exact" if exact else "ld_attn_fwd_bf16")
    return out


def attn_window_plan(N: int, prefix: int, group: int, window: int) -> list:
    """ld_attn_window_plan for every 256-row query block of an N-token sequence [prefix | frames of `group` tokens]: a list of
    (t_lo, t_hi, n_eff) -- the block walks key tiles 0 .. ceil(prefix / 64) - 1 and t_lo .. t_hi - 1 (n_eff tiles).  Host only."""
    lib = _lib.load()
    lo, hi, ne = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    plan = []
    for b in range((N + 255) // 256):
        check(lib.ld_attn_window_plan(N, prefix, group, window, b, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne)),
              "ld_attn_window_plan")
        plan.append((lo.value, hi.value, ne.value))
    return plan


def attn_window_check(N: int, prefix: int, group: int, window: int) -> list:
    """The plan of attn_window_plan, or ValueError with the reason ld_attn_fwd_bf16_window would refuse the shape for (fewer than 6
    key tiles in the sequence or in one block's list): for callers that must know before they launch (ControlDiTRunner)."""
    plan = attn_window_plan(N, prefix, group, window)
    n = (N + ATTN_KEY_TILE - 1) // ATTN_KEY_TILE
    if n < ATTN_PIPELINED_MIN_TILES:
        raise ValueError(f"frame-window attention needs at least {ATTN_PIPELINED_MIN_TILES} key tiles of {ATTN_KEY_TILE}; {N} tokens are {n}")
    short = [(b, p[2]) for b, p in enumerate(plan) if p[2] < ATTN_PIPELINED_MIN_TILES]
    if short:
        raise ValueError(f"frame-window attention (prefix {prefix}, {group} tokens per frame, window {window}): query block {short[0][0]} "
                         f"would walk {short[0][1]} key tiles, the pipelined kernel needs at least {ATTN_PIPELINED_MIN_TILES}")
    return plan


def attn_fwd_window(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, N: int, scale: float,
                    prefix: int, group: int, window: int) -> torch.Tensor:
    """ld_attn_fwd_bf16_window: attn_fwd's unmasked square problem (Nq = Nk = N) where every 256-row query block walks only the
    key tiles of the prefix and of the frames within `window` of its own (attn_window_plan).  Shapes the window form does not
    take raise; nothing runs dense instead."""
    _bf16(q, "q"); _bf16(k, "k"); _bf16(vt, "vt"); _bf16(out, "out")
    B, H, Npad, D = q.shape
    assert D == 64 and k.shape == q.shape and tuple(vt.shape) == (B, H, 64, Npad)
    assert q.is_contiguous() and k.is_contiguous() and vt.is_contiguous() and out.stride(-1) == 1
    assert out.shape[0] == B and out.shape[2] == H * 64 and out.shape[1] >= N
    check(_lib.load().ld_attn_fwd_bf16_window(_ptr(q), _ptr(k), _ptr(vt), _ptr(out), B, H, N, Npad, out.stride(0), out.stride(1),
                                              float(scale), prefix, group, window, _stream()), "ld_attn_fwd_bf16_window")
    return out


def attn_last_fallbacks(out: torch.Tensor) -> torch.Tensor:
    """ld_attn_last_fallbacks: out int32 [1] on the device <- the number of 256-row query blocks of this thread's last attn_fwd launch
    (on the current stream) that left the fast pass's window and were recomputed; 0: kernel without a window, -1: no count kept."""
    assert out.dtype == torch.int32 and out.is_cuda and out.numel() >= 1
    check(_lib.load().ld_attn_last_fallbacks(_ptr(out), _stream()), "ld_attn_last_fallbacks")
    return out


def reset() -> None:
    """ld_reset on the current stream: forget the stream -> counter-set assignments of the dynamic attention launch on the current
    device and zero the sets.  Only when no attention launch is in flight on another stream (after a device synchronise)."""
    check(_lib.load().ld_reset(_stream()), "ld_reset")


def attn_queue_poke(value: int, set_index: int = -1) -> None:
    """Test hook (ld_attn_queue_poke): leave `value` in the attention work-queue counters, as an aborted launch would."""
    check(_lib.load().ld_attn_queue_poke(set_index, value, _stream()), "ld_attn_queue_poke")


# ------------------------------------------------------------------------------------------------
# small-batch / LLM kernels
# ------------------------------------------------------------------------------------------------
def _gemv(symbol, x, w, out, w2, bias, resid, in_act, act, norm_w, norm_eps):
    B, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K and out.shape == (B, N) and x.stride(1) == 1 and out.stride(1) == 1 and w.is_contiguous()
    # the kernels read bias as bf16 always, resid as out's type, norm_w as K floats: another dtype would be misread, not refused
    if bias is not None and bias.dtype != torch.bfloat16:
        raise ValueError(f"{symbol}: bias must be bf16, got {bias.dtype}")
    if resid is not None and resid.dtype != out.dtype:
        raise ValueError(f"{symbol}: resid must have out's dtype {out.dtype}, got {resid.dtype}")
    if w2 is not None and not (w2.dtype == w.dtype and w2.shape == w.shape and w2.is_contiguous()):
        raise ValueError(f"{symbol}: w2 must be contiguous {w.dtype} {tuple(w.shape)} like w, got {w2.dtype} {tuple(w2.shape)}")
    if norm_w is not None and not (norm_w.dtype == torch.float32 and norm_w.numel() == K and norm_w.is_contiguous()):
        raise ValueError(f"{symbol}: norm_w must be contiguous fp32 [{K}], got {norm_w.dtype} {tuple(norm_w.shape)}")
    check(getattr(_lib.load(), symbol)(_ptr(x), x.stride(0), int(x.dtype == torch.float32), _ptr(w), _ptr(w2),
                                       int(w.dtype == torch.float32), _ptr(bias), _ptr(resid),
                                       resid.stride(0) if resid is not None else 0, _ptr(out), out.stride(0),
                                       int(out.dtype == torch.float32), B, N, K, ACT[in_act], ACT[act], _ptr(norm_w), float(norm_eps),
                                       _stream()), symbol)
    return out


def gemv(x, w, out, *, w2=None, bias=None, resid=None, in_act=None, act=None, norm_w=None, norm_eps=0.0):
    """out[B,N] = epi(x[B,K] @ w[N,K]^T) for B <= 4 (weight streaming)."""
    return _gemv("ld_gemv", x, w, out, w2, bias, resid, in_act, act, norm_w, norm_eps)


def gemv_pairs(x, w, out, *, w2=None, bias=None, resid=None, in_act=None, act=None, norm_w=None, norm_eps=0.0):
    """gemv for B = 2 P rows (P <= LLM_MAX_PAIRS samples side by side): rows (2p, 2p+1) get the bits of gemv on those two rows;
    the bf16 register forms stream the weights once for all pairs (ld_gemv_pairs)."""
    return _gemv("ld_gemv_pairs", x, w, out, w2, bias, resid, in_act, act, norm_w, norm_eps)


def gemv_wide(x, w, out, *, w2=None, bias=None, resid=None, in_act=None, act=None, norm_w=None, norm_eps=0.0):
    """gemv for B = 2 P rows, P <= LLM_MAX_WIDE, on the MFMA engine (ld_gemv_wide): bf16 only; a row's bits depend on that row
    alone (not on B or its index); same rounding points as gemv, another order of the fp32 sum."""
    return _gemv("ld_gemv_wide", x, w, out, w2, bias, resid, in_act, act, norm_w, norm_eps)


def rmsnorm(x, w, out, eps):
    rows, D = x.shape
    _bf16(x, "x")
    assert w.dtype == torch.float32 and x.is_contiguous() and out.is_contiguous()
    check(_lib.load().ld_rmsnorm_bf16(_ptr(x), _ptr(w), _ptr(out), rows, D, float(eps), _stream()), "ld_rmsnorm_bf16")
    return out


def layernorm_bf16_to_f32(x, w, b, out, eps):
    rows, D = x.shape
    check(_lib.load().ld_layernorm_bf16_to_f32(_ptr(x), x.stride(0), _ptr(w), _ptr(b), _ptr(out), rows, D, float(eps),
                                               _stream()), "ld_layernorm_bf16_to_f32")
    return out


def llm_rope_append(qkv, cos_t, sin_t, pos, q_out, k_cache, v_cache, B, m, H, Lmax):
    check(_lib.load().ld_llm_rope_append(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), _ptr(pos), _ptr(q_out), _ptr(k_cache),
                                         _ptr(v_cache), B, m, H, Lmax, _stream()), "ld_llm_rope_append")


def llm_kv_attn(q, k_cache, v_cache, pos, out, B, m, H, Lmax, workspace=None, nsplit=1, qkv_fused=None, cos_t=None,
                sin_t=None):
    if workspace is not None and nsplit > 1 and m == 1:
        # split decode attention: B*H*nsplit partial results of 130 words + one arrival counter per (batch row, head) at the tail,
        # which must start at zero (the last arriver re-zeroes it) -- include/landiff_hip.h, ld_llm_kv_attn
        need = B * H * (nsplit * 130 + 1)
        assert workspace.dtype == torch.float32 and workspace.numel() >= need, \
            f"ld_llm_kv_attn workspace: {workspace.numel()} fp32 words, needs B*H*(nsplit*130+1) = {need}"
    check(_lib.load().ld_llm_kv_attn(_ptr(q), _ptr(k_cache), _ptr(v_cache), _ptr(pos), _ptr(out), B, m, H, Lmax,
                                     _ptr(workspace), nsplit, _ptr(qkv_fused), _ptr(cos_t), _ptr(sin_t), _stream()),
          "ld_llm_kv_attn")


def llm_embed(table, token, out):
    B, D = out.shape
    check(_lib.load().ld_llm_embed(_ptr(table), _ptr(token), _ptr(out), B, D, _stream()), "ld_llm_embed")


def llm_layer_table(blocks, k_caches, v_caches):
    """Host-side array of ld_llm_layer for llm_decode_forward (keeps no references: the caller owns the tensors)."""
    arr = (_lib.LlmLayer * len(blocks))()
    for i, w in enumerate(blocks):
        for name in ("wqkv", "wo", "w1", "w3", "w2"):
            assert w[name].dtype == torch.bfloat16 and w[name].is_contiguous()
            setattr(arr[i], name, w[name].data_ptr())
        for name in ("n0", "n1"):
            assert w[name].dtype == torch.float32 and w[name].is_contiguous()
            setattr(arr[i], name, w[name].data_ptr())
        arr[i].k_cache, arr[i].v_cache = k_caches[i].data_ptr(), v_caches[i].data_ptr()
    return arr


LLM_MAX_PAIRS = 4                  # LD_LLM_MAX_PAIRS
LLM_MAX_WIDE = 16                  # LD_LLM_MAX_WIDE


def _llm_decode_forward(symbol, table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b, lnf_out, head, logits,
                        heads, Lmax, nsplit, rms_eps, ln_eps, pos_value):
    B, hidden = x.shape
    for t in (x, qkv, att, gate, lnf_out, logits, head):
        assert t.is_contiguous()
    need = B * heads * (nsplit * 130 + 1)
    assert attn_ws.dtype == torch.float32 and attn_ws.numel() >= need, f"attn_ws: {attn_ws.numel()} words, needs {need}"
    check(getattr(_lib.load(), symbol)(ctypes.addressof(table), len(table), _ptr(emb), _ptr(token), _ptr(pos), int(pos_value), _ptr(x),
                                       _ptr(qkv), _ptr(att), _ptr(gate), _ptr(attn_ws), _ptr(cos_t), _ptr(sin_t), _ptr(lnf_w),
                                       _ptr(lnf_b), _ptr(lnf_out), _ptr(head), _ptr(logits), B, hidden, heads, gate.shape[1],
                                       logits.shape[1], Lmax, nsplit, float(rms_eps), float(ln_eps), _stream()), symbol)


def llm_decode_forward(table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b, lnf_out, head, logits,
                       heads, Lmax, nsplit, rms_eps, ln_eps, pos_value=-1):
    """One decode step (embedding -> all blocks -> final LN -> fp32 head), every launch queued from native code."""
    _llm_decode_forward("ld_llm_decode_forward", table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b, lnf_out, head, logits,
                        heads, Lmax, nsplit, rms_eps, ln_eps, pos_value)


def llm_decode_forward_pairs(table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b, lnf_out, head, logits,
                             heads, Lmax, nsplit, rms_eps, ln_eps, pos_value=-1):
    """llm_decode_forward for P samples of one prompt: B = 2 P rows, pair p = rows (2p, 2p+1); token [P]; nsplit: the value a
    two-row runner with this Lmax uses (ld_llm_decode_forward_pairs)."""
    _llm_decode_forward("ld_llm_decode_forward_pairs", table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b,
                        lnf_out, head, logits, heads, Lmax, nsplit, rms_eps, ln_eps, pos_value)


def llm_decode_forward_wide(table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b, lnf_out, head, logits,
                            heads, Lmax, nsplit, rms_eps, ln_eps, pos_value=-1):
    """llm_decode_forward_pairs on the MFMA engine, P <= LLM_MAX_WIDE samples (ld_llm_decode_forward_wide): the block GEMVs are
    ld_gemv_wide, the head ld_llm_head_f32; pair p's logits depend on pair p alone."""
    _llm_decode_forward("ld_llm_decode_forward_wide", table, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b,
                        lnf_out, head, logits, heads, Lmax, nsplit, rms_eps, ln_eps, pos_value)



LLM_FUSED_CTL_WORDS = 512          # LD_LLM_FUSED_CTL_WORDS


def llm_layer_table_device(table, device):
    """The ld_llm_layer array as a device tensor (the persistent decode kernel reads the table itself)."""
    raw = bytes(memoryview(table).cast("B"))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def llm_decode_forward_fused(table_dev, n_layers, emb, token, pos, x, qkv, att, gate, attn_ws, cos_t, sin_t, lnf_w, lnf_b, lnf_out,
                             head, logits, heads, Lmax, nsplit, rms_eps, ln_eps, ctl):
    """llm_decode_forward with all blocks in one persistent launch (ld_llm_fused.hip); ctl: int32 [LLM_FUSED_CTL_WORDS], zeroed
    before the first step of a decode.  Raises LandiffHipError(unsupported) outside the fused form's shapes."""
    B, hidden = x.shape
    for t in (x, qkv, att, gate, lnf_out, logits, head):
        assert t.is_contiguous()
    assert ctl.dtype == torch.int32 and ctl.numel() >= LLM_FUSED_CTL_WORDS
    check(_lib.load().ld_llm_decode_forward_fused(_ptr(table_dev), n_layers, _ptr(emb), _ptr(token), _ptr(pos), _ptr(x), _ptr(qkv),
                                                  _ptr(att), _ptr(gate), _ptr(attn_ws), _ptr(cos_t), _ptr(sin_t), _ptr(lnf_w),
                                                  _ptr(lnf_b), _ptr(lnf_out), _ptr(head), _ptr(logits), B, hidden, heads,
                                                  gate.shape[1], logits.shape[1], Lmax, nsplit, float(rms_eps), float(ln_eps),
                                                  _ptr(ctl), _stream()), "ld_llm_decode_forward_fused")


LLM_CHAIN_CTL_WORDS = 64 + 256 * 8 * 16     # LD_LLM_CHAIN_CTL_WORDS


def llm_decode_blocks_chained(table, pos_value, x, qkv, att, gate, attn_ws, cos_t, sin_t, heads, Lmax, nsplit, rms_eps, ctl, epoch,
                              stream0, stream1):
    """All blocks of one decode step as dependent launches alternating between two streams (ld_llm_decode_blocks_chained): the
    caller orders stream1 after the producers of the KV cache before the first step and the readers of x after both streams."""
    B, hidden = x.shape
    for t in (x, qkv, att, gate):
        assert t.is_contiguous()
    assert ctl.dtype == torch.int32 and ctl.numel() >= LLM_CHAIN_CTL_WORDS
    check(_lib.load().ld_llm_decode_blocks_chained(ctypes.addressof(table), len(table), int(pos_value), _ptr(x), _ptr(qkv), _ptr(att),
                                                   _ptr(gate), _ptr(attn_ws), _ptr(cos_t), _ptr(sin_t), B, hidden, heads,
                                                   gate.shape[1], Lmax, nsplit, float(rms_eps), _ptr(ctl), int(epoch),
                                                   ctypes.c_void_p(stream0.cuda_stream), ctypes.c_void_p(stream1.cuda_stream)),
          "ld_llm_decode_blocks_chained")


def llm_logits_to_probs(logits, probs, cfg_logits, guided, scale, temperature, pos=None, allowed=None,
                        top_k=None, top_p=None):
    V = probs.shape[-1]
    check(_lib.load().ld_llm_logits_to_probs(_ptr(logits), _ptr(probs), _ptr(cfg_logits), V, int(guided), float(scale),
                                             float(temperature), _ptr(pos), _ptr(allowed),
                                             allowed.stride(0) if allowed is not None else 0,
                                             int(top_k) if top_k is not None else 0,
                                             float(top_p) if top_p is not None else -1.0, _stream()),
          "ld_llm_logits_to_probs")


def llm_sample_advance(logits, probs, cfg_logits, guided, scale, temperature, pos, allowed, noise, forced, token, out_tokens,
                       out_count, sampled, emb, x, top_k=None, top_p=None):
    """probabilities -> draw (argmax(p / noise), noise ~ Exp(1): torch.multinomial's own formula) -> forced-token schedule,
    token record, position advance -> embedding rows of the next token in x: the tail of a decode step in one launch."""
    V = logits.shape[-1]
    B, D = x.shape
    check(_lib.load().ld_llm_sample_advance(_ptr(logits), _ptr(probs), _ptr(cfg_logits), V, int(guided), float(scale),
                                            float(temperature), _ptr(pos), _ptr(allowed),
                                            allowed.stride(0) if allowed is not None else 0,
                                            int(top_k) if top_k is not None else 0,
                                            float(top_p) if top_p is not None else -1.0, _ptr(noise), _ptr(forced),
                                            _ptr(token), _ptr(out_tokens), _ptr(out_count), _ptr(sampled), _ptr(emb),
                                            _ptr(x), B, D, _stream()), "ld_llm_sample_advance")


def _llm_sample_advance_many(symbol, logits, probs, cfg_logits, guided, scale, temperature, pos, allowed, noise, forced, token,
                             out_tokens, out_count, sampled, emb, x, top_k=None, top_p=None):
    V = logits.shape[-1]
    P = noise.shape[0]
    D = x.shape[1]
    assert logits.shape[0] == 2 * P and x.shape[0] == 2 * P and out_tokens.shape[0] == P and out_tokens.stride(1) == 1
    assert pos.numel() == P and token.numel() == P and out_count.numel() == P and (sampled is None or sampled.numel() == P)
    for t in (logits, noise, x, probs, cfg_logits):
        assert t is None or t.is_contiguous()
    check(getattr(_lib.load(), symbol)(_ptr(logits), _ptr(probs), _ptr(cfg_logits), V, int(guided), float(scale), float(temperature),
                                       _ptr(pos), _ptr(allowed), allowed.stride(0) if allowed is not None else 0,
                                       int(top_k) if top_k is not None else 0, float(top_p) if top_p is not None else -1.0,
                                       _ptr(noise), _ptr(forced), _ptr(token), _ptr(out_tokens), out_tokens.stride(0), _ptr(out_count),
                                       _ptr(sampled), _ptr(emb), _ptr(x), P, D, _stream()), symbol)


def llm_sample_advance_pairs(logits, probs, cfg_logits, guided, scale, temperature, pos, allowed, noise, forced, token, out_tokens,
                             out_count, sampled, emb, x, top_k=None, top_p=None):
    """llm_sample_advance for P samples in one launch: logits [2P, V], noise / probs / cfg_logits [P, V], pos / token / out_count /
    sampled [P], out_tokens [P, n], x [2P, D]; forced / allowed are the shared schedule (ld_llm_sample_advance_pairs)."""
    _llm_sample_advance_many("ld_llm_sample_advance_pairs", logits, probs, cfg_logits, guided, scale, temperature, pos, allowed, noise,
                             forced, token, out_tokens, out_count, sampled, emb, x, top_k, top_p)


def llm_sample_advance_wide(logits, probs, cfg_logits, guided, scale, temperature, pos, allowed, noise, forced, token, out_tokens,
                            out_count, sampled, emb, x, top_k=None, top_p=None):
    """llm_sample_advance_pairs with the MFMA engine's cap, P <= LLM_MAX_WIDE (ld_llm_sample_advance_wide): the same kernel."""
    _llm_sample_advance_many("ld_llm_sample_advance_wide", logits, probs, cfg_logits, guided, scale, temperature, pos, allowed, noise,
                             forced, token, out_tokens, out_count, sampled, emb, x, top_k, top_p)



def llm_decode_advance(sampled, forced, pos, token, out_tokens, out_count):
    check(_lib.load().ld_llm_decode_advance(_ptr(sampled), _ptr(forced), _ptr(pos), _ptr(token), _ptr(out_tokens),
                                            _ptr(out_count), _stream()), "ld_llm_decode_advance")


LLM_SAMPLE_MAXV = 4096            # LD_SAMPLE_MAXV


def _f32_rows(t, name, V=None):
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name} must be [rows, cols] with contiguous rows, got shape {tuple(t.shape)} strides {t.stride()}")
    if V is not None and t.shape[1] != V:
        raise ValueError(f"{name} has {t.shape[1]} columns, expected {V}")


def llm_token_logprobs(cond, uncond, target, logprob, guided, scale, temperature, *, pos=None, pos_stride=0, pos_bias=0,
                       allowed=None, forced=None, top_k=None, top_p=None, valid=None, cfg_logits=None):
    """logprob[r] = log-probability of target[r] under the sampler's distribution of logits row r (ld_llm_token_logprobs).
    cond / uncond: fp32 [n, V] views with any row stride (uncond None: unguided); pos: an int32 device word (row r reads
    pos[r * pos_stride]) to which pos_bias is added, or None: row r is position pos_bias + r; allowed [n_pos, w] / forced [n_pos]:
    the schedule tables; target int64 [n], logprob fp32 [n], valid int32 [n] (optional); cfg_logits fp32 [n, V] (optional): the
    guided logits of the rows that are draws."""
    for t in (cond, uncond, target, logprob, pos, allowed, forced, valid, cfg_logits):
        _ptr(t)                                      # CPU tensors are refused before any shape is looked at
    _f32_rows(cond, "cond")
    n, V = cond.shape
    if V > LLM_SAMPLE_MAXV:
        raise ValueError(f"llm_token_logprobs: V = {V} exceeds LD_SAMPLE_MAXV = {LLM_SAMPLE_MAXV}")
    if guided and uncond is None:
        raise ValueError("llm_token_logprobs: guided needs the unconditional rows")
    if uncond is not None:
        _f32_rows(uncond, "uncond", V)
        if uncond.shape[0] != n:
            raise ValueError(f"uncond has {uncond.shape[0]} rows, cond {n}")
    if target.dtype != torch.int64 or target.shape != (n,) or not target.is_contiguous():
        raise ValueError(f"target must be contiguous int64 [{n}], got {target.dtype} {tuple(target.shape)}")
    if logprob.dtype != torch.float32 or logprob.shape != (n,) or not logprob.is_contiguous():
        raise ValueError(f"logprob must be contiguous float32 [{n}], got {logprob.dtype} {tuple(logprob.shape)}")
    if valid is not None and (valid.dtype != torch.int32 or valid.shape != (n,) or not valid.is_contiguous()):
        raise ValueError(f"valid must be contiguous int32 [{n}], got {valid.dtype} {tuple(valid.shape)}")
    if pos is not None and (pos.dtype != torch.int32 or pos.numel() < 1 + (n - 1) * pos_stride or not pos.is_contiguous()):
        raise ValueError(f"pos must be contiguous int32 with {1 + (n - 1) * pos_stride} words, got {pos.dtype} {tuple(pos.shape)}")
    if cfg_logits is not None:
        _f32_rows(cfg_logits, "cfg_logits", V)
        if cfg_logits.shape[0] != n:
            raise ValueError(f"cfg_logits has {cfg_logits.shape[0]} rows, cond {n}")
    n_pos = 0
    if allowed is not None:
        if allowed.dtype != torch.int32 or allowed.dim() != 2 or allowed.stride(1) != 1:
            raise ValueError(f"allowed must be int32 [n_pos, 1 + ids], got {allowed.dtype} {tuple(allowed.shape)}")
        n_pos = allowed.shape[0]
    if forced is not None:
        if forced.dtype != torch.int32 or forced.dim() != 1 or not forced.is_contiguous():
            raise ValueError(f"forced must be contiguous int32 [n_pos], got {forced.dtype} {tuple(forced.shape)}")
        if allowed is not None and forced.shape[0] != n_pos:
            raise ValueError(f"forced has {forced.shape[0]} rows, allowed {n_pos}")
        n_pos = forced.shape[0]
    check(_lib.load().ld_llm_token_logprobs(_ptr(cond), cond.stride(0), _ptr(uncond), uncond.stride(0) if uncond is not None else 0,
                                            n, V, int(guided), float(scale), float(temperature), _ptr(pos), int(pos_stride),
                                            int(pos_bias), _ptr(allowed), allowed.stride(0) if allowed is not None else 0,
                                            _ptr(forced), n_pos, int(top_k) if top_k is not None else 0,
                                            float(top_p) if top_p is not None else -1.0, _ptr(target), _ptr(logprob), _ptr(valid),
                                            _ptr(cfg_logits), cfg_logits.stride(0) if cfg_logits is not None else 0, _stream()), "ld_llm_token_logprobs")
    return logprob


def llm_head_f32(a, w, out):
    """out[M, N] = a[M, K] @ w[N, K]^T, all fp32 with fp32 accumulation (ld_llm_head_f32); a / w / out may have row strides."""
    for t in (a, w, out):
        _ptr(t)
    _f32_rows(a, "a"); _f32_rows(w, "w", a.shape[1]); _f32_rows(out, "out", w.shape[0])
    if out.shape[0] != a.shape[0]:
        raise ValueError(f"out has {out.shape[0]} rows, a {a.shape[0]}")
    M, K = a.shape
    check(_lib.load().ld_llm_head_f32(_ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(out), out.stride(0), M, w.shape[0], K,
                                      _stream()), "ld_llm_head_f32")
    return out


# ------------------------------------------------------------------------------------------------
# normalisation
# ------------------------------------------------------------------------------------------------
def layernorm(x, w, b, out, eps, *, mod=None, mod_bstride=0, shift_img=0, scale_img=0, shift_txt=0, scale_txt=0,
              rows_per_batch=0, text_len=0):
    rows, D = x.shape
    assert x.stride(1) == 1 and out.stride(1) == 1
    check(_lib.load().ld_layernorm(_ptr(x), x.stride(0), int(x.dtype == torch.float32), _ptr(w), _ptr(b), _ptr(out),
                                   out.stride(0), int(out.dtype == torch.float32), rows, D, float(eps), _ptr(mod),
                                   mod_bstride, shift_img, scale_img, shift_txt, scale_txt, rows_per_batch, text_len,
                                   _stream()), "ld_layernorm")
    return out


def layernorm_mxfp8(x, w, b, q, scales, eps, *, mod=None, mod_bstride=0, shift_img=0, scale_img=0, shift_txt=0, scale_txt=0,
                    rows_per_batch=0, text_len=0):
    """layernorm(...) whose bf16 result is written as MXFP8: q uint8 [rows, D], scales uint8 [D/128, rows, 4]."""
    _bf16(x, "x")
    rows, D = x.shape
    assert x.stride(1) == 1 and q.dtype == torch.uint8 and q.shape == (rows, D) and q.stride(1) == 1
    assert scales.dtype == torch.uint8 and tuple(scales.shape) == (D // 128, rows, 4) and scales.is_contiguous()
    check(_lib.load().ld_layernorm_mxfp8(_ptr(x), x.stride(0), _ptr(w), _ptr(b), _ptr(q), q.stride(0), _ptr(scales),
                                         rows, rows, D, float(eps), _ptr(mod), mod_bstride, shift_img, scale_img,
                                         shift_txt, scale_txt, rows_per_batch, text_len, _stream()), "ld_layernorm_mxfp8")
    return q, scales


def feature_norm_cl(features, mean, std, out, T, C, P):
    """features [T,C,h,w] (fp32/bf16) -> out [T*P, C] bf16 = (x - mean[c]) / (std[c] + 1e-8)."""
    assert features.is_contiguous() and out.is_contiguous() and out.dtype == torch.bfloat16
    assert features.dtype in (torch.float32, torch.bfloat16) and mean.dtype == torch.float32 and std.dtype == torch.float32
    check(_lib.load().ld_feature_norm_cl(_ptr(features), int(features.dtype == torch.float32), _ptr(mean), _ptr(std), _ptr(out),
                                         T, C, P, _stream()), "ld_feature_norm_cl")


def feature_denorm(x, mean, std, out=None):
    """x bf16 [rows, C] -> bf16(float(x) * (std[c] + 1e-8) + mean[c]) (VideoVQ.denorm_features when a mean_std_path is configured)."""
    _bf16(x, "x")
    assert x.is_contiguous() and mean.dtype == torch.float32 and std.dtype == torch.float32
    out = x if out is None else out
    assert out.is_contiguous() and out.dtype == torch.bfloat16 and out.shape == x.shape
    check(_lib.load().ld_feature_denorm(_ptr(x), _ptr(mean), _ptr(std), _ptr(out), x.shape[0], x.shape[1], _stream()),
          "ld_feature_denorm")
    return out


def vq_nearest(x, codebook, idx, dim):
    """x bf16 [rows, >=dim], codebook fp32 [V, dim] -> idx int64 [rows] (first code at minimum Euclidean distance)."""
    _bf16(x, "x")
    assert codebook.dtype == torch.float32 and codebook.is_contiguous() and codebook.shape[1] == dim
    assert idx.dtype == torch.int64 and idx.is_contiguous() and x.stride(1) == 1
    check(_lib.load().ld_vq_nearest(_ptr(x), x.stride(0), _ptr(codebook), _ptr(idx), x.shape[0], codebook.shape[0], dim,
                                    _stream()), "ld_vq_nearest")


def gemm_qkv_heads(a, w, bias, q, k, vt, B, N, H, Npad, ln, eps=1e-6):
    """The DiT qkv Linear with the head split in its epilogue: a [B*N, K] -> q, k [B,H,Npad,64] (QK-LayerNorm with
    ln = (q_w, q_b, k_w, k_b)) and vt [B,H,64,Npad].  Rows [N, Npad) of q / k / vt are left as they are (keep them zero)."""
    _bf16(a, "a"); _bf16(w, "w")
    assert a.shape[0] == B * N and w.shape == (3 * H * 64, a.shape[1]) and a.stride(1) == 1 and w.is_contiguous()
    assert q.shape == (B, H, Npad, 64) and k.shape == q.shape and vt.shape == (B, H, 64, Npad)
    assert q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    check(_lib.load().ld_gemm_qkv_heads(_ptr(a), a.stride(0), _ptr(w), _ptr(bias), B * N, a.shape[1], _ptr(q), _ptr(k), _ptr(vt),
                                        B, N, H, Npad, _ptr(ln[0]), _ptr(ln[1]), _ptr(ln[2]), _ptr(ln[3]), float(eps), _stream()),
          "ld_gemm_qkv_heads")


def gemm_qkv_heads_mxfp8(a8, sa, w8, sw, bias, q, k, vt, B, N, H, Npad, ln, eps=1e-6):
    """gemm_qkv_heads on MXFP8 operands: a8 uint8 [B*N, K] + scales sa [K/128, B*N, 4], w8 [3*H*64, K] + sw [K/128, 3*H*64, 4]."""
    assert a8.dtype == torch.uint8 and w8.dtype == torch.uint8 and a8.stride(1) == 1 and w8.is_contiguous()
    M, K = a8.shape
    assert M == B * N and w8.shape == (3 * H * 64, K) and tuple(sa.shape) == (K // 128, M, 4) and tuple(sw.shape) == (K // 128, 3 * H * 64, 4)
    assert sa.is_contiguous() and sw.is_contiguous() and sa.dtype == torch.uint8 and sw.dtype == torch.uint8
    assert q.shape == (B, H, Npad, 64) and k.shape == q.shape and vt.shape == (B, H, 64, Npad)
    assert q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    check(_lib.load().ld_gemm_qkv_heads_mxfp8(_ptr(a8), a8.stride(0), _ptr(sa), _ptr(w8), _ptr(sw), _ptr(bias), M, K, _ptr(q), _ptr(k), _ptr(vt),
                                              B, N, H, Npad, _ptr(ln[0]), _ptr(ln[1]), _ptr(ln[2]), _ptr(ln[3]), float(eps), _stream()),
          "ld_gemm_qkv_heads_mxfp8")


def qkv_split(qkv, q, k, vt, B, N, H, Npad, *, ln=None, rope=None, eps=1e-6):
    """ln = (q_w, q_b, k_w, k_b) for the DiT QK-LayerNorm, or rope = (cos, sin) [N,32] fp32 for TiTok; neither: the plain
    split (mode 2, the Theia ViT)."""
    assert ln is None or rope is None
    mode = 0 if ln is not None else 1 if rope is not None else 2
    lw = ln if ln is not None else (None,) * 4
    rp = rope if rope is not None else (None, None)
    check(_lib.load().ld_qkv_split(_ptr(qkv), _ptr(q), _ptr(k), _ptr(vt), B, N, H, Npad, mode, _ptr(lw[0]), _ptr(lw[1]),
                                   _ptr(lw[2]), _ptr(lw[3]), float(eps), _ptr(rp[0]), _ptr(rp[1]), _stream()),
          "ld_qkv_split")


def groupnorm_stats(x, stats, F, P, C, G):
    """stats [F, G, 2] float64 <- (sum, sum of squares) per frame-group and channel group; deterministic (fixed-order
    reduction of per-workgroup partials through a workspace from torch's caching allocator)."""
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == F * G * 2
    lib = _lib.load()
    ws = torch.empty(F * int(lib.ld_groupnorm_stats_blocks(P)) * G * 2, device=stats.device, dtype=torch.float64)
    check(lib.ld_groupnorm_stats(_ptr(x), _ptr(stats), _ptr(ws), F, P, C, G, _stream()), "ld_groupnorm_stats")


GN_FOLD_BLOCKS = 256      # ld_norm_group.hip: LD_GN_FOLD_BLOCKS


def groupnorm_stats_from_conv(part, stats, P, C, G):
    """stats [1, G, 2] float64 <- the partial sums conv_cl(..., gn_partials=True) left behind (P output rows, C channels);
    deterministic (fixed-order fold + reduce)."""
    assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() == G * 2
    assert part.dtype == torch.float32 and part.is_contiguous() and part.numel() == (P + 63) // 64 * (C // 4) * 2
    ws = torch.empty(GN_FOLD_BLOCKS * G * 2, device=stats.device, dtype=torch.float64)
    check(_lib.load().ld_groupnorm_stats_from_conv(_ptr(part), _ptr(stats), _ptr(ws), P, C, G, _stream()),
          "ld_groupnorm_stats_from_conv")


def groupnorm_apply(x, out_padded, stats, gamma, beta, F, T, H, W, C, G, *, zy=None, zb=None, zshape=(1, 1, 1),
                    tpad=0, hpad=0, wpad=0, swish=True, eps=1e-6):
    check(_lib.load().ld_groupnorm_apply(_ptr(x), _ptr(out_padded), _ptr(stats), _ptr(gamma), _ptr(beta), _ptr(zy), _ptr(zb),
                                         F, T, H, W, C, G, zshape[0], zshape[1], zshape[2], tpad, hpad, wpad, int(swish),
                                         float(eps), _stream()), "ld_groupnorm_apply")


# ------------------------------------------------------------------------------------------------
# layout / elementwise
# ------------------------------------------------------------------------------------------------
def patchify(x, sem, out, p):
    B, T, C, H, W = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    check(_lib.load().ld_patchify(_ptr(x), _ptr(sem), _ptr(out), B, T, C, H, W, p, _stream()), "ld_patchify")


def unpatchify_cfg(lin, x, out, p, c_out, c_skip, scale):
    _, T, C, H, W = x.shape
    check(_lib.load().ld_unpatchify_cfg(_ptr(lin), _ptr(x), _ptr(out), T, C, H, W, p, float(c_out), float(c_skip),
                                        float(scale), _stream()), "ld_unpatchify_cfg")


def axpbypcz(out, x, a, y=None, b=0.0, z=None, c=0.0):
    check(_lib.load().ld_axpbypcz(_ptr(out), _ptr(x), float(a), _ptr(y), float(b), _ptr(z), float(c), out.numel(),
                                  _stream()), "ld_axpbypcz")
    return out


# ---- clip editing (ld_edit.hip) ----------------------------------------------------------------------
def _keep_mask(mask, name):
    if mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"{name}: the mask must be uint8 or bool, got {mask.dtype}")
    if mask.dim() != 3 or not mask.is_contiguous():
        raise ValueError(f"{name}: the mask must be a contiguous 3-d tensor, got {tuple(mask.shape)}")


def latent_pin(x, known, noise=None, mask=None, alpha=1.0, sigma=0.0):
    """In place on x [T, C, H, W] fp32 (leading 1s allowed): where mask [T, H, W] (uint8 / bool, broadcast over C; None: everywhere)
    is set, x = alpha * known + sigma * noise with separately rounded products -- or x = known, a copy, with noise None.  Elsewhere
    x keeps its bits.  noise may be x itself."""
    if x.dim() < 4 or any(s != 1 for s in x.shape[:-4]):
        raise ValueError(f"latent_pin: x must be [T, C, H, W] (leading 1s allowed), got {tuple(x.shape)}")
    T, C, H, W = x.shape[-4:]
    for t, name in ((x, "x"), (known, "known"), (noise, "noise")):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise TypeError(f"latent_pin: {name} must be float32, got {t.dtype}")
        if t.shape != x.shape or not t.is_contiguous():
            raise ValueError(f"latent_pin: {name} must be contiguous and of x's shape {tuple(x.shape)}, got {tuple(t.shape)}")
    if mask is not None:
        _keep_mask(mask, "latent_pin")
        if tuple(mask.shape) != (T, H, W):
            raise ValueError(f"latent_pin: the mask must be [{T}, {H}, {W}] for x {tuple(x.shape)}, got {tuple(mask.shape)}")
    check(_lib.load().ld_latent_pin(_ptr(x), _ptr(known), _ptr(noise), _ptr(mask), float(alpha), float(sigma), T, C, H, W, _stream()),
          "ld_latent_pin")
    return x


def mask_to_latent(mask_px, out=None):
    """Pixel keep-mask [F, Hp, Wp] (uint8 / bool, non-zero = keep) -> latent keep-mask uint8 [(F + 3) // 4, Hp // 8, Wp // 8]: a cell
    is kept only if every pixel of its block is (frames {0} / {4t-3 .. 4t}, an 8 x 8 tile).  F % 4 != 1, Hp % 8 or Wp % 8: refused."""
    _keep_mask(mask_px, "mask_to_latent")
    F, Hp, Wp = mask_px.shape
    if out is None:
        out = torch.empty((F + 3) // 4, Hp // 8, Wp // 8, dtype=torch.uint8, device=mask_px.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != ((F + 3) // 4, Hp // 8, Wp // 8) or not out.is_contiguous():
        raise ValueError(f"mask_to_latent: out must be contiguous uint8 [{(F + 3) // 4}, {Hp // 8}, {Wp // 8}], got {out.dtype} {tuple(out.shape)}")
    check(_lib.load().ld_mask_to_latent(_ptr(mask_px), _ptr(out), F, Hp, Wp, _stream()), "ld_mask_to_latent")
    return out


def _resize_geometry(name, src, dims, out_hw, frame_idx, box, filter):
    """The shared argument checks of resize_u8 / resize_mask_u8 -> (Fs, Hs, Ws, n_out, Ho, Wo, box, device frame_idx, filter id)."""
    from .conform import FILTERS
    if src.dim() != dims or not src.is_contiguous():
        raise ValueError(f"{name}: the source must be a contiguous {dims}-d tensor, got {tuple(src.shape)}")
    Fs, Hs, Ws = src.shape[:3]
    Ho, Wo = (int(v) for v in out_hw)
    if min(Fs, Hs, Ws, Ho, Wo) < 1:
        raise ValueError(f"{name}: empty shape (source {tuple(src.shape)}, target {Ho} x {Wo})")
    if filter not in FILTERS:
        raise ValueError(f"{name}: filter must be one of {tuple(FILTERS)}, got {filter!r}")
    box = (0, 0, Hs, Ws) if box is None else tuple(int(v) for v in box)
    y0, x0, hc, wc = box
    if y0 < 0 or x0 < 0 or hc < 1 or wc < 1 or y0 + hc > Hs or x0 + wc > Ws:
        raise ValueError(f"{name}: the crop box {box} leaves the {Hs} x {Ws} source")
    idx = None
    n_out = Fs
    if frame_idx is not None:
        host = [int(v) for v in (frame_idx.tolist() if hasattr(frame_idx, "tolist") else frame_idx)]
        if not host or min(host) < 0 or max(host) >= Fs:
            raise ValueError(f"{name}: frame_idx must be a non-empty list of indices in [0, {Fs}), got {host[:8]}{'...' if len(host) > 8 else ''}")
        n_out = len(host)
        if host != list(range(Fs)):                 # (the identity needs no table)
            idx = torch.tensor(host, dtype=torch.int32).to(src.device)
    return Fs, Hs, Ws, n_out, Ho, Wo, box, idx, FILTERS[filter]


def _axis_tables(n_in, n_out, filter, device, weights=True):
    from .conform import axis_table
    win, w = axis_table(n_in, n_out, filter)
    return torch.from_numpy(win).to(device), (torch.from_numpy(w).to(device) if weights else None)


def resize_u8(src, out_hw, *, frame_idx=None, box=None, filter="bilinear", out=None):
    """Antialiased resampling of uint8 channels-last frames [Fs, Hs, Ws, C] (C 1 or 3) -> uint8 [n_out, Ho, Wo, C]: output frame k
    is made from the crop box (y0, x0, h, w) of source frame frame_idx[k] (a host list; None: every frame in order).  PyTorch's
    antialias weights (conform.axis_table), fp32 accumulation, one clamp(round-half-even) at the end; only the box is read."""
    if src.dtype != torch.uint8:
        raise TypeError(f"resize_u8: the source must be uint8, got {src.dtype}")
    if src.dim() == 4 and src.shape[3] not in (1, 3):
        raise ValueError(f"resize_u8: C must be 1 or 3, got {tuple(src.shape)}")
    Fs, Hs, Ws, n_out, Ho, Wo, box, idx, fid = _resize_geometry("resize_u8", src, 4, out_hw, frame_idx, box, filter)
    C = src.shape[3]
    if out is None:
        out = torch.empty(n_out, Ho, Wo, C, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n_out, Ho, Wo, C) or not out.is_contiguous():
        raise ValueError(f"resize_u8: out must be contiguous uint8 [{n_out}, {Ho}, {Wo}, {C}], got {out.dtype} {tuple(out.shape)}")
    win_y, w_y = _axis_tables(box[2], Ho, filter, src.device)
    win_x, w_x = _axis_tables(box[3], Wo, filter, src.device)
    check(_lib.load().ld_resize_u8(_ptr(src), _ptr(out), _ptr(idx), _ptr(win_y), _ptr(w_y), w_y.shape[1], _ptr(win_x), _ptr(w_x),
                                   w_x.shape[1], Fs, Hs, Ws, C, n_out, Ho, Wo, *box, fid, _stream()), "ld_resize_u8")
    return out


def resize_mask_u8(mask, out_hw, *, frame_idx=None, box=None, filter="bilinear", out=None):
    """A keep-mask [Fs, Hs, Ws] (uint8 / bool, non-zero = keep) through resize_u8's geometry -> uint8 [n_out, Ho, Wo], 1 where every
    source pixel in the output pixel's tap window [lo_y, hi_y) x [lo_x, hi_x) of `filter` is non-zero, else 0."""
    if mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"resize_mask_u8: the mask must be uint8 or bool, got {mask.dtype}")
    Fs, Hs, Ws, n_out, Ho, Wo, box, idx, fid = _resize_geometry("resize_mask_u8", mask, 3, out_hw, frame_idx, box, filter)
    if out is None:
        out = torch.empty(n_out, Ho, Wo, dtype=torch.uint8, device=mask.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n_out, Ho, Wo) or not out.is_contiguous():
        raise ValueError(f"resize_mask_u8: out must be contiguous uint8 [{n_out}, {Ho}, {Wo}], got {out.dtype} {tuple(out.shape)}")
    win_y, _ = _axis_tables(box[2], Ho, filter, mask.device, weights=False)
    win_x, _ = _axis_tables(box[3], Wo, filter, mask.device, weights=False)
    check(_lib.load().ld_resize_mask_u8(_ptr(mask), _ptr(out), _ptr(idx), _ptr(win_y), _ptr(win_x), Fs, Hs, Ws, n_out, Ho, Wo, *box,
                                        fid, _stream()), "ld_resize_mask_u8")
    return out


def retime_u8(frames, src_idx, phase_p, q, search, penalty, max_sad, want_motion=False):
    """uint8 channels-last frames [F, H, W, C] (C 1 or 3) -> uint8 [n_out, H, W, C]: output frame k lies at source position
    src_idx[k] + phase_p[k] / q (host lists).  Phase 0 copies; every other frame is block-matched and motion-compensated between
    its two neighbours in integer arithmetic (landiff_amd.retime states the parameters).  want_motion: also the
    motion field int16 [n_out, ceil(H/8), ceil(W/8), 2] = (dy, dx) and the SAD int32 [n_out, ceil(H/8), ceil(W/8)].  One launch on the
    current stream; does not synchronise."""
    from .retime import MAX_Q, check_search
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise TypeError(f"retime_u8: the frames must be a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() != 4 or not frames.is_contiguous() or min(frames.shape) < 1 or frames.shape[3] not in (1, 3):
        raise ValueError(f"retime_u8: the frames must be a non-empty contiguous [F, H, W, C] with C 1 or 3, got {tuple(frames.shape)}")
    F, H, W, C = frames.shape
    check_search(search, penalty, max_sad, "retime_u8")
    if isinstance(q, bool) or int(q) != q or not 1 <= q <= MAX_Q:
        raise ValueError(f"retime_u8: q must be an integer in 1..{MAX_Q}, got {q!r}")
    idx = [int(v) for v in (src_idx.tolist() if hasattr(src_idx, "tolist") else src_idx)]
    ph = [int(v) for v in (phase_p.tolist() if hasattr(phase_p, "tolist") else phase_p)]
    if not idx or len(idx) != len(ph):
        raise ValueError(f"retime_u8: src_idx and phase_p must be non-empty lists of one length, got {len(idx)} and {len(ph)}")
    for k, (i, p) in enumerate(zip(idx, ph)):
        if not 0 <= p < q:
            raise ValueError(f"retime_u8: phase_p[{k}] = {p} is not in [0, {q})")
        if i < 0 or i + (p > 0) > F - 1:
            raise ValueError(f"retime_u8: output frame {k} at source position {i} + {p}/{q} leaves the clip's {F} frames")
    n_out = len(idx)
    tab = torch.tensor([idx, ph], dtype=torch.int32).to(frames.device)
    out = torch.empty(n_out, H, W, C, dtype=torch.uint8, device=frames.device)
    nby, nbx = -(-H // 8), -(-W // 8)
    mv = torch.empty(n_out, nby, nbx, 2, dtype=torch.int16, device=frames.device) if want_motion else None
    sad = torch.empty(n_out, nby, nbx, dtype=torch.int32, device=frames.device) if want_motion else None
    check(_lib.load().ld_retime_u8(_ptr(frames), _ptr(out), _ptr(tab[0]), _ptr(tab[1]), int(q), _ptr(mv), _ptr(sad), F, n_out, H, W, C,
                                   int(search), int(penalty), int(max_sad), _stream()), "ld_retime_u8")
    return (out, mv, sad) if want_motion else out


def _jpeg_sub(name, subsampling) -> int:
    if subsampling not in ("420", "444"):
        raise ValueError(f"{name}: subsampling must be '420' or '444', got {subsampling!r}")
    return int(subsampling)


def _jpeg_size(symbol, *args) -> int:
    """One of the library's *_size questions: the answer, or its refusal raised."""
    n = getattr(_lib.load(), symbol)(*args)
    if n < 0:
        check(int(n), symbol)
    return int(n)


def jpeg_size(what: int, F, H, W, subsampling: str, header_bytes: int = 0) -> int:
    """ld_jpeg_size: 0 blocks per frame, 1 segments (MCU rows) per frame, 2 blocks per segment, 3 the most bytes of a segment, 4 the
    most bytes of F streams with their headers (include/landiff_hip.h, LD_JPEG_SIZE_*).  Needs no GPU."""
    return _jpeg_size("ld_jpeg_size", int(what), int(F), int(H), int(W), _jpeg_sub("jpeg_size", subsampling), int(header_bytes))


def _jpeg_frames(name, frames, quality):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise TypeError(f"{name}: the frames must be a uint8 tensor, got {getattr(frames, 'dtype', type(frames))}")
    if frames.dim() != 4 or min(frames.shape) < 1 or frames.shape[3] != 3 or frames.stride(3) != 1 or frames.stride(2) != 3:
        raise ValueError(f"{name}: the frames must be a non-empty [F, H, W, 3] with contiguous pixels (rows and frames may be strided), "
                         f"got {tuple(frames.shape)} with strides {tuple(frames.stride()) if frames.dim() == 4 else None}")
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"{name}: quality must be an integer in 1..100, got {quality!r}")
    return tuple(int(v) for v in frames.shape[:3])


def jpeg_coefs_u8(frames, quality: int, subsampling: str = "420"):
    """uint8 RGB frames [F, H, W, 3] -> the quantised DCT coefficients int16 [F, blocks, 64] of their baseline JPEG, blocks in scan
    order, coefficients in zigzag order.  One launch on the current stream; does not synchronise."""
    from .encode import device_tables
    F, H, W = _jpeg_frames("jpeg_coefs_u8", frames, quality)
    sub = _jpeg_sub("jpeg_coefs_u8", subsampling)
    coefs = torch.empty(F, jpeg_size(0, F, H, W, subsampling), 64, dtype=torch.int16, device=frames.device)
    check(_lib.load().ld_jpeg_coefs_u8(_ptr(frames), frames.stride(0), frames.stride(1), _ptr(device_tables(frames.device)), _ptr(coefs),
                                       F, H, W, sub, int(quality), _stream()), "ld_jpeg_coefs_u8")
    return coefs


def jpeg_entropy_i16(coefs, mcus_per_row: int, subsampling: str = "420"):
    """coefficients int16 [n_seg, mcus_per_row * (6 | 3), 64] (every row of dim 0 one segment: an MCU row) -> (segs uint8
    [n_seg, capacity], seg_len int64 [n_seg]): the entropy-coded, stuffed bytes of every segment, without markers.  Two launches."""
    from .encode import device_tables
    sub = _jpeg_sub("jpeg_entropy_i16", subsampling)
    bpm = 6 if sub == 420 else 3
    if not isinstance(coefs, torch.Tensor) or coefs.dtype != torch.int16:
        raise TypeError(f"jpeg_entropy_i16: the coefficients must be an int16 tensor, got {getattr(coefs, 'dtype', type(coefs))}")
    if coefs.dim() != 3 or not coefs.is_contiguous() or coefs.shape[0] < 1 or coefs.shape[1] != mcus_per_row * bpm or coefs.shape[2] != 64:
        raise ValueError(f"jpeg_entropy_i16: the coefficients must be a contiguous [n_seg, {mcus_per_row} * {bpm}, 64], got {tuple(coefs.shape)}")
    n_seg = int(coefs.shape[0])
    cap = jpeg_size(3, 1, 8, int(mcus_per_row) * (16 if sub == 420 else 8), subsampling)
    segs = torch.empty(n_seg, cap, dtype=torch.uint8, device=coefs.device)
    seg_len = torch.empty(n_seg, dtype=torch.int64, device=coefs.device)
    check(_lib.load().ld_jpeg_entropy_i16(_ptr(coefs), _ptr(device_tables(coefs.device)), _ptr(segs), cap, _ptr(seg_len), n_seg,
                                          int(mcus_per_row), sub, _stream()), "ld_jpeg_entropy_i16")
    return segs, seg_len


_JPEG_HEADERS: dict = {}


def _jpeg_header_on(device, H, W, quality, subsampling):
    """encode.jpeg_header of such frames as a uint8 tensor on the device, cached."""
    from .encode import jpeg_header
    key = (str(device), H, W, int(quality), subsampling)
    if key not in _JPEG_HEADERS:
        if len(_JPEG_HEADERS) > 64:
            _JPEG_HEADERS.clear()
        _JPEG_HEADERS[key] = torch.frombuffer(bytearray(jpeg_header(H, W, int(quality), subsampling)), dtype=torch.uint8).to(device)
    return _JPEG_HEADERS[key]


def _jpeg_encode_buffers(device, F, H, W, subsampling, header):
    """What both encode wrappers allocate -> (capacity, coefficients int16 [F, blocks, 64], seg_ws int64 [2, segments], out uint8 [capacity])."""
    cap = jpeg_size(4, F, H, W, subsampling, header.numel())
    coefs = torch.empty(F, jpeg_size(0, F, H, W, subsampling), 64, dtype=torch.int16, device=device)
    seg_ws = torch.empty(2, F * jpeg_size(1, F, H, W, subsampling), dtype=torch.int64, device=device)
    return cap, coefs, seg_ws, torch.empty(cap, dtype=torch.uint8, device=device)


def jpeg_encode_u8(frames, quality: int, subsampling: str = "420"):
    """uint8 RGB frames [F, H, W, 3] -> (stream buffer uint8 [capacity], offsets int64 [F], lengths int64 [F]), all on the device:
    frame f's complete baseline JPEG is buffer[offsets[f] : offsets[f] + lengths[f]], the frames back to back.  The buffer is sized
    by ld_jpeg_size's bound (nothing is ever cut to fit); only the streams' bytes of it are touched.  Four launches on the current
    stream; does not synchronise."""
    from .encode import device_tables
    F, H, W = _jpeg_frames("jpeg_encode_u8", frames, quality)
    sub = _jpeg_sub("jpeg_encode_u8", subsampling)
    dev = frames.device
    header = _jpeg_header_on(dev, H, W, quality, subsampling)
    cap, coefs, seg_ws, out = _jpeg_encode_buffers(dev, F, H, W, subsampling, header)
    table = torch.empty(2, F, dtype=torch.int64, device=dev)
    check(_lib.load().ld_jpeg_encode_u8(_ptr(frames), frames.stride(0), frames.stride(1), _ptr(device_tables(dev)), _ptr(header),
                                        header.numel(), _ptr(coefs), _ptr(seg_ws), _ptr(out), cap, _ptr(table[0]), _ptr(table[1]),
                                        F, H, W, sub, int(quality), _stream()), "ld_jpeg_encode_u8")
    return out, table[0], table[1]


def jpeg_rate_size(what: int, F, H, W, subsampling: str, q_min: int, q_max: int) -> int:
    """ld_jpeg_rate_size: 0 the rounds of the search 1 + ceil(log2(q_max - q_min + 1)), 1 the launches of ld_jpeg_encode_rate_u8, 2 the
    int32 words of its state workspace, 3 the int64 words of its trial table (include/landiff_hip.h, LD_JPEG_RATE_SIZE_*).  Needs no GPU."""
    return _jpeg_size("ld_jpeg_rate_size", int(what), int(F), int(H), int(W), _jpeg_sub("jpeg_rate_size", subsampling), int(q_min), int(q_max))


def jpeg_c8_u8(frames, subsampling: str = "420"):
    """uint8 RGB frames [F, H, W, 3] -> c8 int16 [F, blocks, 64]: jpeg_coefs_u8 up to the quantiser (8 x the DCT coefficient, |c8| <=
    8192), in its layout.  One launch on the current stream; does not synchronise."""
    from .encode import device_tables
    F, H, W = _jpeg_frames("jpeg_c8_u8", frames, 1)
    sub = _jpeg_sub("jpeg_c8_u8", subsampling)
    if not frames.is_cuda:
        raise ValueError("jpeg_c8_u8: the frames must be on the GPU, got a CPU tensor")
    c8 = torch.empty(F, jpeg_size(0, F, H, W, subsampling), 64, dtype=torch.int16, device=frames.device)
    check(_lib.load().ld_jpeg_c8_u8(_ptr(frames), frames.stride(0), frames.stride(1), _ptr(device_tables(frames.device)), _ptr(c8),
                                    F, H, W, sub, _stream()), "ld_jpeg_c8_u8")
    return c8


def jpeg_quant_i16(c8, quality, subsampling: str = "420"):
    """c8 int16 [F, blocks, 64] (jpeg_c8_u8) and quality int32 [F] on the same device, every entry in 1..100 -> the quantised
    coefficients int16 [F, blocks, 64]: frame f's are jpeg_coefs_u8's at quality[f].  One launch; the qualities are not read on the
    host, so keeping them in range is the caller's."""
    from .encode import device_tables
    sub = _jpeg_sub("jpeg_quant_i16", subsampling)
    bpm = 6 if sub == 420 else 3
    if not isinstance(c8, torch.Tensor) or c8.dtype != torch.int16:
        raise TypeError(f"jpeg_quant_i16: c8 must be an int16 tensor, got {getattr(c8, 'dtype', type(c8))}")
    if not isinstance(quality, torch.Tensor) or quality.dtype != torch.int32:
        raise TypeError(f"jpeg_quant_i16: quality must be an int32 tensor, got {getattr(quality, 'dtype', type(quality))}")
    if not c8.is_cuda or quality.device != c8.device:
        raise ValueError(f"jpeg_quant_i16: c8 and quality must be on one GPU, got {c8.device} and {quality.device}")
    if c8.dim() != 3 or not c8.is_contiguous() or min(c8.shape) < 1 or c8.shape[1] % bpm or c8.shape[2] != 64:
        raise ValueError(f"jpeg_quant_i16: c8 must be a contiguous [F, blocks (a multiple of {bpm}), 64], got {tuple(c8.shape)}")
    if quality.dim() != 1 or quality.shape[0] != c8.shape[0] or not quality.is_contiguous():
        raise ValueError(f"jpeg_quant_i16: quality must be a contiguous [{c8.shape[0]}], got {tuple(quality.shape)}")
    coefs = torch.empty_like(c8)
    check(_lib.load().ld_jpeg_quant_i16(_ptr(c8), _ptr(device_tables(c8.device)), _ptr(quality), _ptr(coefs), int(c8.shape[0]),
                                        int(c8.shape[1]), sub, _stream()), "ld_jpeg_quant_i16")
    return coefs


def jpeg_encode_rate_u8(frames, q_max: int, subsampling: str = "420", frame_bytes=None, clip_bytes=None, q_min: int = 1):
    """jpeg_encode_u8 under a byte budget: exactly one of frame_bytes (every stream <= it, a quality per frame) and
    clip_bytes (the streams together <= it, one quality); the qualities are searched in q_min..q_max on the device.  -> (stream
    buffer uint8 [capacity], table int64 [4 + 2 R, F]), both on the device: table[0] offsets, [1] lengths, [2] qualities, [3]
    over_budget, table[4:].view(R, F, 2) the (quality, size) of every trial.  1 + 3 R + 4 launches on the current stream; does not
    synchronise."""
    from .encode import device_tables, jpeg_dqt_offsets
    name = "jpeg_encode_rate_u8"
    F, H, W = _jpeg_frames(name, frames, q_max)
    sub = _jpeg_sub(name, subsampling)
    if isinstance(q_min, bool) or int(q_min) != q_min or not 1 <= q_min <= q_max:
        raise ValueError(f"{name}: q_min must be an integer in 1..q_max = {q_max}, got {q_min!r}")
    if (frame_bytes is None) == (clip_bytes is None):
        raise ValueError(f"{name}: give exactly one of frame_bytes and clip_bytes, got {frame_bytes!r} and {clip_bytes!r}")
    budget = frame_bytes if clip_bytes is None else clip_bytes
    if isinstance(budget, bool) or int(budget) != budget or budget < 1:
        raise ValueError(f"{name}: the budget must be an integer >= 1, got {budget!r}")
    if not frames.is_cuda:
        raise ValueError(f"{name}: the frames must be on the GPU, got a CPU tensor")
    dev = frames.device
    header = _jpeg_header_on(dev, H, W, q_max, subsampling)
    dqt = jpeg_dqt_offsets()
    R = jpeg_rate_size(0, F, H, W, subsampling, q_min, q_max)
    cap, coefs, seg_ws, out = _jpeg_encode_buffers(dev, F, H, W, subsampling, header)
    c8 = torch.empty_like(coefs)
    state = torch.empty(jpeg_rate_size(2, F, H, W, subsampling, q_min, q_max), dtype=torch.int32, device=dev)
    table = torch.empty(4 + 2 * R, F, dtype=torch.int64, device=dev)
    check(_lib.load().ld_jpeg_encode_rate_u8(_ptr(frames), frames.stride(0), frames.stride(1), _ptr(device_tables(dev)), _ptr(header),
                                             header.numel(), dqt[0], dqt[1], _ptr(c8), _ptr(coefs), _ptr(seg_ws), _ptr(state),
                                             _ptr(out), cap, _ptr(table[0]), _ptr(table[1]), _ptr(table[2]), _ptr(table[3]),
                                             _ptr(table[4]), 2 * R * F, F, H, W, sub, int(q_min), int(q_max),
                                             int(frame_bytes or 0), int(clip_bytes or 0), _stream()), "ld_jpeg_encode_rate_u8")
    return out, table


def jpeg_dec_size(what: int, H, W, subsampling: str) -> int:
    """ld_jpeg_dec_size: 0 blocks per frame, 1 MCUs per frame, 2 bytes of the plane workspace per frame, 3 words of a table set
    (include/landiff_hip.h, LD_JPEG_DEC_SIZE_*).  Needs no GPU."""
    return _jpeg_size("ld_jpeg_dec_size", int(what), int(H), int(W), _jpeg_sub("jpeg_dec_size", subsampling))


def _jpeg_dec_arg(name, what, t, dtype, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{name}: {what} must be a contiguous {dtype} tensor, got {getattr(t, 'dtype', type(t))}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {what} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _jpeg_dec_tables(name, tables, H, W, subsampling):
    words = jpeg_dec_size(3, H, W, subsampling)
    if _jpeg_dec_arg(name, "tables", tables, torch.int32).dim() != 2 or tables.shape[0] < 1 or tables.shape[1] != words:
        raise ValueError(f"{name}: tables must be [n_sets, {words}], got {tuple(tables.shape)}")


def _jpeg_dec_inputs(name, data, seg_table, frame_info, ri, tables, tset, H, W, subsampling):
    """What both entropy routes check of their inputs -> (F, S, the library's subsampling code)."""
    sub = _jpeg_sub(name, subsampling)
    _jpeg_dec_arg(name, "data", data, torch.uint8)
    F = int(_jpeg_dec_arg(name, "ri", ri, torch.int32).numel())
    if seg_table.dim() != 3 or F < 1:
        raise ValueError(f"{name}: the segment table must be [F, rows, 5], got {tuple(seg_table.shape)}")
    S = int(seg_table.shape[1])
    _jpeg_dec_arg(name, "seg_table", seg_table, torch.int64, (F, S, 5))
    _jpeg_dec_arg(name, "frame_info", frame_info, torch.int64, (F, 3))
    _jpeg_dec_arg(name, "tset", tset, torch.int32, (F,))
    _jpeg_dec_tables(name, tables, H, W, subsampling)
    return F, S, sub


def jpeg_find_segments(data, scan, ri, n_rows: int, H: int, W: int, subsampling: str = "420"):
    """data uint8 [n] (the frames' streams), scan int64 [F, 2] (where each frame's entropy-coded data starts, the bytes to search),
    ri int32 [F] (restart intervals in MCUs, 0 = none) -> (segment table int64 [F, n_rows, 5], frame info int64 [F, 3]) as
    include/landiff_hip.h states them.  n_rows >= the most segments a frame has.  One launch; does not synchronise."""
    name = "jpeg_find_segments"
    sub = _jpeg_sub(name, subsampling)
    _jpeg_dec_arg(name, "data", data, torch.uint8)
    F = int(_jpeg_dec_arg(name, "ri", ri, torch.int32).numel())
    _jpeg_dec_arg(name, "scan", scan, torch.int64, (F, 2))
    if data.dim() != 1 or ri.dim() != 1 or F < 1 or int(n_rows) < 1:
        raise ValueError(f"{name}: data [n], ri [F] with F >= 1 and n_rows >= 1 are expected, got {tuple(data.shape)}, {tuple(ri.shape)}, {n_rows}")
    seg = torch.empty(F, int(n_rows), 5, dtype=torch.int64, device=data.device)
    info = torch.empty(F, 3, dtype=torch.int64, device=data.device)
    check(_lib.load().ld_jpeg_find_segments(_ptr(data), data.numel(), _ptr(scan), _ptr(ri), _ptr(seg), _ptr(info), F, int(n_rows),
                                            int(H), int(W), sub, _stream()), "ld_jpeg_find_segments")
    return seg, info


def jpeg_decode_entropy(data, seg_table, frame_info, ri, tables, tset, H: int, W: int, subsampling: str = "420"):
    """The segments of jpeg_find_segments -> (coefficients int16 [F, blocks, 64] in ld_jpeg_coefs_u8's layout, status int32 [F, rows],
    decode.STATUS per segment).  tables int32 [n_sets, words] (decode.decode_tables), tset int32 [F] the set of every frame.  One
    launch, one lane per segment; does not synchronise."""
    F, S, sub = _jpeg_dec_inputs("jpeg_decode_entropy", data, seg_table, frame_info, ri, tables, tset, H, W, subsampling)
    coefs = torch.empty(F, jpeg_dec_size(0, H, W, subsampling), 64, dtype=torch.int16, device=data.device)
    status = torch.empty(F, S, dtype=torch.int32, device=data.device)
    check(_lib.load().ld_jpeg_decode_entropy(_ptr(data), data.numel(), _ptr(seg_table), _ptr(frame_info), _ptr(ri), _ptr(tables),
                                             _ptr(tset), int(tables.shape[0]), _ptr(coefs), _ptr(status), F, S, int(H), int(W), sub,
                                             _stream()), "ld_jpeg_decode_entropy")
    return coefs, status


def jpeg_dec_sync_size(what: int, scan_bytes: int, F: int, S: int, sub_bytes: int = 256, max_rounds: int = 32) -> int:
    """ld_jpeg_dec_sync_size: 0 bytes of jpeg_decode_entropy_sync's workspace, 1 rows of its flat list of subsequences (and of the
    exit table), from what the host knows: the frames' summed scan bytes, F frames of at most S segments.  Needs no GPU."""
    return _jpeg_size("ld_jpeg_dec_sync_size", int(what), int(scan_bytes), int(F), int(S), int(sub_bytes), int(max_rounds))


def jpeg_decode_entropy_sync(data, seg_table, frame_info, ri, tables, tset, H: int, W: int, subsampling: str = "420",
                             sub_bytes: int = 256, max_rounds: int = 32, return_exits: bool = False, scan_bytes=None):
    """jpeg_decode_entropy by the second route: one lane per subsequence of sub_bytes raw bytes of a segment, for
    streams without restart markers -> (coefficients, status, sync_info int32 [F, rows, 2] = (rounds to the fixed point, 1 if the
    segment fell back to the lane-per-segment kernel)[, (exits int64 [subsequences, 4] = (p, j, k, blocks), index int32 [F, rows, 2]
    = (first row, rows) of every segment)]).  Coefficients and status are jpeg_decode_entropy's whatever max_rounds is.
    scan_bytes: the frames' summed scan bytes where the caller knows them (default: all of data); it sizes the grids.  A fixed
    number of launches; does not synchronise."""
    F, S, sub = _jpeg_dec_inputs("jpeg_decode_entropy_sync", data, seg_table, frame_info, ri, tables, tset, H, W, subsampling)
    scan_bytes = data.numel() if scan_bytes is None else min(int(scan_bytes), data.numel())
    ws_bytes = jpeg_dec_sync_size(0, scan_bytes, F, S, sub_bytes, max_rounds)
    dev = data.device
    coefs = torch.empty(F, jpeg_dec_size(0, H, W, subsampling), 64, dtype=torch.int16, device=dev)
    status = torch.empty(F, S, dtype=torch.int32, device=dev)
    sync_info = torch.empty(F, S, 2, dtype=torch.int32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    exits = index = None
    if return_exits:
        exits = torch.zeros(jpeg_dec_sync_size(1, scan_bytes, F, S, sub_bytes, max_rounds), 4, dtype=torch.int64, device=dev)
        index = torch.empty(F, S, 2, dtype=torch.int32, device=dev)
    check(_lib.load().ld_jpeg_decode_entropy_sync(_ptr(data), data.numel(), _ptr(seg_table), _ptr(frame_info), _ptr(ri), _ptr(tables),
                                                  _ptr(tset), int(tables.shape[0]), _ptr(coefs), _ptr(status), F, S, int(H), int(W), sub,
                                                  scan_bytes, int(sub_bytes), int(max_rounds), _ptr(ws), ws_bytes, _ptr(sync_info),
                                                  _ptr(exits) if return_exits else None, _ptr(index) if return_exits else None,
                                                  _stream()), "ld_jpeg_decode_entropy_sync")
    return (coefs, status, sync_info, (exits, index)) if return_exits else (coefs, status, sync_info)


def jpeg_decode_rgb(coefs, tables, tset, H: int, W: int, subsampling: str = "420", out=None):
    """coefficients int16 [F, blocks, 64] -> uint8 frames [F, H, W, 3] (out: a uint8 [F, H, W, 3] whose rows and frames may be
    strided, e.g. a window of a wider buffer).  Two launches; does not synchronise."""
    name = "jpeg_decode_rgb"
    sub = _jpeg_sub(name, subsampling)
    blocks = jpeg_dec_size(0, H, W, subsampling)
    if not isinstance(coefs, torch.Tensor) or coefs.dim() != 3:
        raise TypeError(f"{name}: the coefficients must be an int16 tensor [F, {blocks}, 64]")
    F = int(coefs.shape[0])
    _jpeg_dec_arg(name, "coefs", coefs, torch.int16, (F, blocks, 64))
    _jpeg_dec_arg(name, "tset", tset, torch.int32, (F,))
    _jpeg_dec_tables(name, tables, H, W, subsampling)
    if out is None:
        out = torch.empty(F, int(H), int(W), 3, dtype=torch.uint8, device=coefs.device)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (F, int(H), int(W), 3)
            or out.stride(3) != 1 or out.stride(2) != 3):
        raise ValueError(f"{name}: out must be uint8 [{F}, {H}, {W}, 3] with contiguous pixels (rows and frames may be strided)")
    planes = torch.empty(F, jpeg_dec_size(2, H, W, subsampling), dtype=torch.uint8, device=coefs.device)
    check(_lib.load().ld_jpeg_decode_rgb(_ptr(coefs), _ptr(tables), _ptr(tset), int(tables.shape[0]), _ptr(planes), _ptr(out),
                                         out.stride(0), out.stride(1), F, int(H), int(W), sub, _stream()), "ld_jpeg_decode_rgb")
    return out


SSIM_TAPS, SSIM_SIGMA = 11, 1.5                      # LD_SSIM_TAPS of include/landiff_hip.h
SSIM_TILE_H, SSIM_TILE_ELEMS = 32, 48               # LD_SSIM_TILE_H / LD_SSIM_TILE_ELEMS: they size the workspace, which the library checks


def ssim_window() -> np.ndarray:
    """The 11-tap Gaussian of sigma 1.5, normalised to sum 1 in float64 and rounded to fp32 once: the table ld_clip_ssim_u8 takes."""
    x = np.arange(SSIM_TAPS, dtype=np.float64) - (SSIM_TAPS - 1) / 2
    g = np.exp(-(x * x) / (2.0 * SSIM_SIGMA * SSIM_SIGMA))
    return (g / g.sum()).astype(np.float32)


_SSIM_WINDOWS: dict = {}


def _clip_pair(name, a, b, mask):
    """The shared argument checks of clip_diff_u8 / clip_ssim_u8 -> (a, b, mask as uint8 or None), contiguous."""
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise ValueError(f"{name}: the clips must be uint8 tensors, got {getattr(t, 'dtype', type(t))}")
    if a.dim() != 4 or a.shape[3] not in (1, 3) or min(a.shape) < 1:
        raise ValueError(f"{name}: a clip must be a non-empty [F, H, W, C] with C 1 or 3, got {tuple(a.shape)}")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{name}: the clips must have one shape, got {tuple(a.shape)} and {tuple(b.shape)} (nothing is resized)")
    if a.device != b.device:
        raise ValueError(f"{name}: the clips must be on one device, got {a.device} and {b.device}")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
            raise ValueError(f"{name}: the mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}")
        if tuple(mask.shape) != tuple(a.shape[:3]):
            raise ValueError(f"{name}: the mask must be {tuple(a.shape[:3])} for clips {tuple(a.shape)}, got {tuple(mask.shape)}")
        if mask.device != a.device:
            raise ValueError(f"{name}: the mask must be on the clips' device {a.device}, got {mask.device}")
        mask = mask.contiguous().view(torch.uint8)
    return a.contiguous(), b.contiguous(), mask


def clip_diff_u8(a, b, mask=None):
    """Exact integer statistics of two uint8 clips [F, H, W, C] (C 1 or 3) -> int64 [F, C, 5]: the number of counted pixels, sum
    (a-b)^2, sum |a-b|, max |a-b| and the number of pixels with a != b, per frame and channel, over the pixels the bool mask
    [F, H, W] keeps (None: all).  Runs on the current stream; does not synchronise."""
    a, b, mask = _clip_pair("clip_diff_u8", a, b, mask)
    F, H, W, C = a.shape
    out = torch.empty(F, C, 5, dtype=torch.int64, device=a.device)
    check(_lib.load().ld_clip_diff_u8(_ptr(a), _ptr(b), _ptr(mask), _ptr(out), F, H, W, C, _stream()), "ld_clip_diff_u8")
    return out


def clip_ssim_u8(a, b, mask=None):
    """SSIM of two uint8 clips [F, H, W, C] (C 1 or 3; H, W >= 11) -> float64 [F, C, 2]: the sum of the SSIM map's values and their
    count per frame and channel (11-tap Gaussian window of sigma 1.5, valid region, L = 255: DESIGN 8.10), over the map positions
    whose centre pixel the bool mask [F, H, W] keeps (None: all).  Runs on the current stream; does not synchronise."""
    a, b, mask = _clip_pair("clip_ssim_u8", a, b, mask)
    F, H, W, C = a.shape
    tiles = -(-max(H - SSIM_TAPS + 1, 1) // SSIM_TILE_H) * -(-max(W - SSIM_TAPS + 1, 1) // (SSIM_TILE_ELEMS // C))
    win = _SSIM_WINDOWS.get(a.device)
    if win is None:                                 # uploaded once per device: a call then copies nothing from the host
        win = _SSIM_WINDOWS[a.device] = torch.from_numpy(ssim_window()).to(a.device)
    ws = torch.empty(F * tiles * C * 2, dtype=torch.float64, device=a.device)
    out = torch.empty(F, C, 2, dtype=torch.float64, device=a.device)
    check(_lib.load().ld_clip_ssim_u8(_ptr(a), _ptr(b), _ptr(mask), _ptr(win), _ptr(out), _ptr(ws), ws.numel(), F, H, W, C, _stream()),
          "ld_clip_ssim_u8")
    return out


def timestep_embedding(t, out, max_period=10000.0):
    B, dim = out.shape
    check(_lib.load().ld_timestep_embedding(_ptr(t), _ptr(out), B, dim, float(max_period), _stream()),
          "ld_timestep_embedding")


def place_cl(x, out_padded, F, Ti, Hi, Wi, Cin, Cout, *, mode=0, time_up=False, tpad=0, hpad=1, wpad=1):
    check(_lib.load().ld_place_cl(_ptr(x), _ptr(out_padded), F, Ti, Hi, Wi, Cin, Cout, mode, int(time_up), tpad, hpad,
                                  wpad, _stream()), "ld_place_cl")


def to_uint8(x, out, video, P):
    check(_lib.load().ld_to_uint8(_ptr(x), x.stride(-2), _ptr(out), _ptr(video), P, _stream()), "ld_to_uint8")


def latent_to_cl(x, out, T, C, H, W, Cpad, mul, src_tchw):
    check(_lib.load().ld_latent_to_cl(_ptr(x), _ptr(out), T, C, H, W, Cpad, float(mul), int(src_tchw), _stream()),
          "ld_latent_to_cl")


# ---- DiT step cache (ld_dit_cache.hip) ---------------------------------------------------------------
DIT_CACHE_WS_FLOATS = 4096         # LD_DIT_CACHE_WS_FLOATS of include/landiff_hip.h


def _cache_operands(name, *tensors):
    """Same-shape contiguous bf16 tensors (None entries skipped) -> their element count."""
    first = tensors[0]
    for t in tensors:
        if t is None:
            continue
        _bf16(t, name)
        if not t.is_contiguous() or t.shape != first.shape:
            raise ValueError(f"{name}: operands must be contiguous and of one shape, got {tuple(t.shape)} beside {tuple(first.shape)}")
    if first.numel() < 1:
        raise ValueError(f"{name}: empty operands")
    return first.numel()


def _cache_sums(name, out, workspace, device):
    if out is None:
        out = torch.empty(2, device=device, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty(DIT_CACHE_WS_FLOATS, device=device, dtype=torch.float32)
    for t, n in ((out, 2), (workspace, DIT_CACHE_WS_FLOATS)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"{name}: out / workspace must be contiguous float32 of at least 2 / {DIT_CACHE_WS_FLOATS} elements")
    return out, workspace


def absdiff_sums(cur, prev, out=None, workspace=None, update_prev=False):
    """out f32 [2] = (sum|cur - prev|, sum|prev|) over bf16 tensors of one shape, fp32 sums that repeat bit for bit.
    update_prev: the same pass writes prev <- cur (the sums are those against the old prev)."""
    n = _cache_operands("absdiff_sums", cur, prev)
    out, workspace = _cache_sums("absdiff_sums", out, workspace, cur.device)
    check(_lib.load().ld_absdiff_sums(_ptr(cur), _ptr(prev), n, _ptr(out), _ptr(workspace), int(bool(update_prev)), _stream()),
          "ld_absdiff_sums")
    return out


def residual_sub(a, b, out=None, old=None, out2=None, workspace=None):
    """out = bf16(float(a) - float(b)).  With old (which may be `out` itself, read before it is overwritten): returns
    (out, out2) with out2 f32 [2] = (sum|out - old|, sum|old|); without: returns out."""
    if out is None:
        out = torch.empty_like(a)
    n = _cache_operands("residual_sub", a, b, out, old)
    if old is None:
        check(_lib.load().ld_residual_sub(_ptr(a), _ptr(b), _ptr(out), n, None, None, None, _stream()), "ld_residual_sub")
        return out
    out2, workspace = _cache_sums("residual_sub", out2, workspace, a.device)
    check(_lib.load().ld_residual_sub(_ptr(a), _ptr(b), _ptr(out), n, _ptr(old), _ptr(out2), _ptr(workspace), _stream()),
          "ld_residual_sub")
    return out, out2


def residual_add(a, r, out=None):
    """out = bf16(float(a) + float(r)); out may be a (in place)."""
    if out is None:
        out = torch.empty_like(a)
    n = _cache_operands("residual_add", a, r, out)
    check(_lib.load().ld_residual_add(_ptr(a), _ptr(r), _ptr(out), n, _stream()), "ld_residual_add")
    return out


# ---- DiT CFG branch skipping (ld_dit_guidance.hip) ---------------------------------------------------
DIT_GUIDANCE_WS_FLOATS = 5120      # LD_DIT_GUIDANCE_WS_FLOATS of include/landiff_hip.h


def _guidance_f32(name, x, *tensors):
    """x [1, T, C, H, W] (or [T, C, H, W]) contiguous fp32; the other tensors (None skipped) fp32, contiguous, of x's element count."""
    for t in (x,) + tensors:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != x.numel():
            raise ValueError(f"{name}: x / out / delta must be contiguous float32 of one size, got {tuple(t.shape)} {t.dtype}")
    return tuple(x.shape[-4:])


def unpatchify_cfg_keep(lin, x, out, delta, p, c_out, c_skip, scale, delta_old=None, sums=None, workspace=None):
    """A full CFG step that keeps its difference: out = d_u + scale * delta with delta = d_c - d_u (out: the bits of unpatchify_cfg).
    delta_old (may be `delta` itself, read before it is overwritten) or None.  Returns sums f32 [5] = (sum e_u e_c, sum e_u^2,
    sum e_c^2, sum|delta - delta_old|, sum|delta_old|), fp32 sums that repeat bit for bit; the last two are 0 without delta_old."""
    T, C, H, W = _guidance_f32("unpatchify_cfg_keep", x, out, delta, delta_old)
    _bf16(lin, "lin")
    if not lin.is_contiguous() or lin.numel() != 2 * x.numel():
        raise ValueError(f"unpatchify_cfg_keep: lin must be contiguous [2, n_img, C*p*p], got {tuple(lin.shape)}")
    if sums is None:
        sums = torch.empty(5, device=x.device, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty(DIT_GUIDANCE_WS_FLOATS, device=x.device, dtype=torch.float32)
    for t, n in ((sums, 5), (workspace, DIT_GUIDANCE_WS_FLOATS)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"unpatchify_cfg_keep: sums / workspace must be contiguous float32 of at least 5 / {DIT_GUIDANCE_WS_FLOATS} elements")
    check(_lib.load().ld_unpatchify_cfg_keep(_ptr(lin), _ptr(x), _ptr(out), _ptr(delta), _ptr(delta_old), _ptr(sums), _ptr(workspace),
                                             T, C, H, W, p, float(c_out), float(c_skip), float(scale), _stream()),
          "ld_unpatchify_cfg_keep")
    return sums


def unpatchify_cond(lin_cond, x, out, p, c_out, c_skip, scale=1.0, delta=None):
    """A cond-only step: out = d_c (delta None) or d_c + (scale - 1) * delta (the kept difference of an earlier full step)."""
    T, C, H, W = _guidance_f32("unpatchify_cond", x, out, delta)
    _bf16(lin_cond, "lin_cond")
    if not lin_cond.is_contiguous() or lin_cond.numel() != x.numel():
        raise ValueError(f"unpatchify_cond: lin_cond must be contiguous [n_img, C*p*p], got {tuple(lin_cond.shape)}")
    check(_lib.load().ld_unpatchify_cond(_ptr(lin_cond), _ptr(x), _ptr(out), _ptr(delta), T, C, H, W, p, float(c_out), float(c_skip),
                                         float(scale), _stream()), "ld_unpatchify_cond")
    return out


# ---- 3D-VAE encoder (ld_vae_enc.hip) ----------------------------------------------------------------
def vae_enc_place_input(frames, out_padded):
    """frames uint8 / f32 [F, H, W, 3] -> out_padded bf16 [F+2, H+2, W+2, Cpad] (every element written)."""
    assert frames.dtype in (torch.uint8, torch.float32) and frames.is_contiguous() and frames.shape[-1] == 3
    F, H, W, _ = frames.shape
    _bf16(out_padded, "out_padded")
    assert out_padded.is_contiguous() and tuple(out_padded.shape[:3]) == (F + 2, H + 2, W + 2)
    check(_lib.load().ld_vae_enc_place_input(_ptr(frames), int(frames.dtype == torch.uint8), _ptr(out_padded), F, H, W,
                                             out_padded.shape[3], _stream()), "ld_vae_enc_place_input")
    return out_padded


def vae_enc_downsample_out_frames(T: int, compress_time: bool) -> int:
    return ((T + 1) // 2 if T % 2 else T // 2) if compress_time and T > 1 else T


def vae_enc_downsample(x, out, T, H, W, C, compress_time):
    """x bf16 [T*H*W, C] -> out bf16 [To, H/2+2, W/2+2, 4C] (time pool + space-to-depth; every element written)."""
    _bf16(x, "x"); _bf16(out, "out")
    To = vae_enc_downsample_out_frames(T, compress_time)
    assert x.is_contiguous() and x.numel() == T * H * W * C and out.is_contiguous()
    assert tuple(out.shape) == (To, H // 2 + 2, W // 2 + 2, 4 * C), (out.shape, To, H, W, C)
    check(_lib.load().ld_vae_enc_downsample(_ptr(x), _ptr(out), T, H, W, C, int(compress_time), _stream()),
          "ld_vae_enc_downsample")
    return out


def vae_posterior(x, z, T, Z, H, W, scale, eps=None, mean=None, logvar=None):
    """x f32 [T*H*W, >= 2Z] -> z f32 [T, Z, H, W] = scale * (mean [+ exp(0.5 logvar) * eps]); eps f32 [Z, T, H, W]."""
    assert x.dtype == torch.float32 and x.stride(1) == 1 and x.shape[0] == T * H * W and x.shape[1] >= 2 * Z
    for t in (z, eps, mean, logvar):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == T * Z * H * W)
    check(_lib.load().ld_vae_posterior(_ptr(x), x.stride(0), _ptr(eps), _ptr(z), _ptr(mean), _ptr(logvar), T, Z, H, W,
                                       float(scale), _stream()), "ld_vae_posterior")
    return z

# ---- T5 text encoders -------------------------------------------------------------------------------
def t5_rmsnorm(x, w, out, eps):
    _bf16(x, "x"); _bf16(w, "w"); _bf16(out, "out")
    rows, D = x.shape
    check(_lib.load().ld_t5_rmsnorm(_ptr(x), _ptr(w), _ptr(out), rows, D, float(eps), _stream()), "ld_t5_rmsnorm")
    return out


def t5_attn(q, k, v, out, bias_table, bucket, H):
    """q, k, v, out: [N, ld] bf16 views (last dim contiguous, same row stride); bucket int32 [2N-1]."""
    N = q.shape[0]
    ld = q.stride(0)
    assert k.stride(0) == ld and v.stride(0) == ld and out.stride(0) == ld and bucket.dtype == torch.int32
    check(_lib.load().ld_t5_attn(_ptr(q), _ptr(k), _ptr(v), _ptr(out), ld, _ptr(bias_table), _ptr(bucket), N, H, _stream()),
          "ld_t5_attn")
    return out


# ---- Theia feature extractor (ld_theia.hip) ----------------------------------------------------------------
def vit_patch_rows(frames, out, S, nhwc):
    """uint8 frames [T,3,S,S] (nhwc=False) or [T,H,W,3] with H, W <= S (nhwc=True, grey-127 square padding made on the fly)
    -> out bf16 [T*(S/16)^2, 768] im2col rows of the patch Conv2d, bf16((u - 127.5) / 127.5)."""
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4
    _bf16(out, "out")
    T = frames.shape[0]
    H, W = (frames.shape[1], frames.shape[2]) if nhwc else (frames.shape[2], frames.shape[3])
    assert (frames.shape[3] == 3) if nhwc else (frames.shape[1] == 3)
    assert out.is_contiguous() and tuple(out.shape) == (T * (S // 16) ** 2, 768)
    check(_lib.load().ld_vit_patch_rows(_ptr(frames), int(nhwc), _ptr(out), T, H, W, S, _stream()), "ld_vit_patch_rows")
    return out


def vit_embed(patch, pos, x, T, P):
    """patch bf16 [T*P, C], pos f32 [1+P, C] (row 0 = CLS + its position) -> x f32 [T*(1+P), C]."""
    _bf16(patch, "patch")
    C = patch.shape[1]
    assert patch.is_contiguous() and patch.shape[0] == T * P
    assert pos.dtype == torch.float32 and pos.is_contiguous() and tuple(pos.shape) == (1 + P, C)
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (T * (1 + P), C)
    check(_lib.load().ld_vit_embed(_ptr(patch), _ptr(pos), _ptr(x), T, P, C, _stream()), "ld_vit_embed")
    return x


def vit_tail(x, ln_w, ln_b, eps, T, s, gh, gw, feat=None, cl=None, mean=None, std=None):
    """x f32 [T*(1+s*s), C] -> final LayerNorm, CLS dropped, crop / zero pad of the s x s grid to (gh, gw): feat f32 [T,C,gh,gw]
    and / or cl bf16 [T*gh*gw, C] = bf16((feat - mean) / (std + 1e-8)) channels-last."""
    C = x.shape[1]
    N = 1 + s * s
    assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (T * N, C)
    assert ln_w.dtype == torch.float32 and ln_b.dtype == torch.float32 and ln_w.numel() == C and ln_b.numel() == C
    if feat is not None:
        assert feat.dtype == torch.float32 and feat.is_contiguous() and tuple(feat.shape) == (T, C, gh, gw)
    if cl is not None:
        _bf16(cl, "cl")
        assert cl.is_contiguous() and tuple(cl.shape) == (T * gh * gw, C)
        assert mean.dtype == torch.float32 and std.dtype == torch.float32 and mean.numel() == C and std.numel() == C
    check(_lib.load().ld_vit_tail(_ptr(x), _ptr(ln_w), _ptr(ln_b), float(eps), T, N, s, gh, gw, C, _ptr(feat), _ptr(cl),
                                  _ptr(mean), _ptr(std), _stream()), "ld_vit_tail")
