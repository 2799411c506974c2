"""Frame-window attention (ld_attn_fwd_bf16_window: ld_attn_q64_win_kernel / ld_attn_q64_win_dyn_kernel), key by key.

The rule is restated here (rule(), not imported from the product): per 256-row query block, the key tiles of the prefix and of the
frames within w of the block's own; every row of the block sees exactly the keys k < N of the listed tiles.  Every launch asserts
which kernel ran and writes into NaN-sentinel output with three extra rows behind row N of every batch that must come back
untouched.  Designs:

  * count: Q = 0, so every visible key has p = 1 exactly; V is a one-hot of class(k), out[q][d] = count_d(q) / total(q) with exact
    integer sums, roundings 1 / total, one multiply and the bf16 store (2^-8 relative), counts <= 32: round(out * total) recovers
    every count.  class = k % 64 counts the tiles, class = (k // 32) % 64 names the half tiles read (<= 64 of them at these shapes):
    a wrong tile shift, a dropped or a leaked key moves an integer;
  * bit identity: the window launch walks, per block, the same logical iteration as the dense kernel on that block's tiles gathered
    into a contiguous zero-padded copy -- the same bits;
  * random N(0, 1) data against an fp32 torch softmax over the dense mask of the rule, with the bound of tests/test_gpu_attn.py for
    this kernel (max abs error < 2e-2).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN16 = 0x7FA5                      # sentinel bit pattern (a quiet bf16 NaN)
EXTRA_ROWS = 3
SCALE = 0.125

# (N, P, G, w): ragged last tile, frames straddling tiles and blocks; no prefix; everything on tile / block boundaries
CASES = [(1890, 90, 200, 0), (1890, 90, 200, 1), (2000, 100, 190, 1), (1000, 0, 125, 1), (2048, 128, 320, 1)]


def rule(N, P, G, w):
    """-> per 256-row query block the list of key tiles it walks (the rule, restated)."""
    n, pt = -(-N // 64), -(-P // 64)
    blocks = []
    for b in range(-(-N // 256)):
        r0 = 256 * b
        r1 = min(r0 + 256, N) - 1
        if r0 < P:
            blocks.append(list(range(n)))
            continue
        f_lo, f_hi = (r0 - P) // G, (r1 - P) // G
        k_lo, k_hi = P + max(0, f_lo - w) * G, min(N, P + (f_hi + w + 1) * G)
        t_lo, t_hi = max(pt, k_lo // 64), -(-k_hi // 64)
        blocks.append(list(range(pt)) + list(range(t_lo, t_hi)))
    return blocks


@functools.lru_cache(maxsize=None)
def dense_mask(N, P, G, w):
    """bool [N, N] on the host: row r sees key k."""
    m = np.zeros((N, N), bool)
    for b, tiles in enumerate(rule(N, P, G, w)):
        cols = np.zeros(N, bool)
        for t in tiles:
            cols[64 * t:min(64 * t + 64, N)] = True
        m[256 * b:min(256 * b + 256, N)] = cols
    return m


def test_cases_are_what_they_claim():
    """Host arithmetic only: the shapes cross the seams the cases are there for, and every list is legal (>= 6 tiles)."""
    assert [len(t) for t in rule(1890, 90, 200, 0)] == [30, 11, 9, 10, 10, 12, 9, 6]
    assert [len(t) for t in rule(1890, 90, 200, 1)] == [30, 14, 16, 16, 16, 19, 12, 9]
    for N, P, G, w in CASES + [(2048, 128, 240, 1)]:
        lists = rule(N, P, G, w)
        assert -(-N // 64) >= 6 and min(len(t) for t in lists) >= 6, (N, P, G, w)
        assert -(-N // 32) <= 64                                        # the half-tile one-hot names every half tile
        assert any(len(t) < -(-N // 64) for t in lists)                 # the window skips something
        assert any(t[-1] < -(-N // 64) - 1 for t in lists)              # ... and some list ends before the last tile
    assert any(t[-(-100 // 64)] > -(-100 // 64) for t in rule(2000, 100, 190, 1))      # a list with a gap behind the prefix tiles
    assert 1890 % 64 and 2000 % 64 and 1000 % 64 and 2048 % 256 == 0 and 128 % 64 == 0 and 320 % 64 == 0


def _last_kernel():
    from landiff_amd import _lib
    return (_lib.load().ld_attn_last_kernel() or b"").decode()


def _pad(x, Npad):                  # [B, H, N, 64] -> zero-padded [B, H, Npad, 64]
    B, H, N, D = x.shape
    out = torch.zeros(B, H, Npad, D, device=x.device, dtype=x.dtype)
    out[:, :, :N] = x
    return out


def _randn(cuda, B, H, N, seed, q_scale=1.0, spike=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    q = (torch.randn(B, H, N, 64, generator=g) * q_scale).to(cuda, BF)
    k = torch.randn(B, H, N, 64, generator=g).to(cuda, BF)
    v = torch.randn(B, H, N, 64, generator=g).to(cuda, BF)
    if spike:
        k[:, :, N - 3] = q[:, :, 5] * 4
    return q, k, v


def _packed(q, k, v):
    Npad = (q.shape[2] + 127) // 128 * 128
    return _pad(q, Npad), _pad(k, Npad), _pad(v, Npad).transpose(2, 3).contiguous()


def _sentinel(cuda, B, N, H):
    return torch.full((B, N + EXTRA_ROWS, H * 64), NAN16, device=cuda, dtype=torch.int16).view(BF)


def _check_sentinel(buf, N):
    raw = buf.view(torch.int16)
    assert (raw[:, N:] == NAN16).all(), "rows behind row N were written"
    assert not torch.isnan(buf[:, :N].float()).any(), "a row of [0, N) was left unwritten (or came out NaN)"


def _window(qp, kp, vt, N, P, G, w, expect="ld_attn_q64_win_kernel"):
    """One window launch into a sentinel buffer -> out [B, N, H * 64] (a view of it)."""
    from landiff_amd import ops
    B, H = qp.shape[:2]
    buf = _sentinel(qp.device, B, N, H)
    ops.attn_fwd_window(qp, kp, vt, buf[:, :N], N, SCALE, P, G, w)
    assert _last_kernel() == expect
    torch.cuda.synchronize()
    _check_sentinel(buf, N)
    return buf[:, :N]


def _reference(q, k, v, N, P, G, w):
    """fp32 torch softmax over the dense mask of the rule -> [B, N, H * 64] fp32."""
    B, H = q.shape[:2]
    mask = torch.from_numpy(dense_mask(N, P, G, w)).to(q.device)
    s = (q.float() @ k.float().transpose(-1, -2)) * SCALE
    s = s.masked_fill(~mask, float("-inf"))
    return (torch.softmax(s, -1) @ v.float()).permute(0, 2, 1, 3).reshape(B, N, H * 64)


@pytest.mark.parametrize("N,P,G,w", CASES)
def test_exact_key_membership(cuda, N, P, G, w):
    """Check 1: counts of visible keys per class, for two one-hot V designs, equal the rule's for every row."""
    B, H = 1, 2
    mask = dense_mask(N, P, G, w)
    total = mask.sum(1)
    g = torch.Generator(device="cpu").manual_seed(N + w)
    k = torch.randn(B, H, N, 64, generator=g).to(cuda, BF)
    q = torch.zeros_like(k)
    ar = np.arange(N)
    for cls in (ar % 64, (ar // 32) % 64):
        onehot = np.zeros((N, 64), np.float32)
        onehot[ar, cls] = 1.0
        v = torch.from_numpy(onehot).to(cuda, BF)[None, None].expand(B, H, N, 64).contiguous()
        out = _window(*_packed(q, k, v), N, P, G, w)
        want = mask.astype(np.float32) @ onehot                         # [N, 64] integer counts
        assert want.max() <= 32
        got = out.float().cpu().numpy().reshape(B, N, H, 64) * total[None, :, None, None]
        assert np.array_equal(np.rint(got), np.broadcast_to(want[None, :, None, :], got.shape))
        assert np.abs(got - np.rint(got)).max() < 0.25


def _gathered_dense(qp, kp, vt, N, tiles):
    """The dense kernel on the keys of `tiles` gathered into a contiguous zero-padded copy -> out [B, N, H * 64]."""
    from landiff_amd import ops
    B, H, Npad, _ = qp.shape
    kg, vg = torch.zeros_like(kp), torch.zeros_like(vt)
    for j, t in enumerate(tiles):
        kg[:, :, 64 * j:64 * j + 64] = kp[:, :, 64 * t:64 * t + 64]
        vg[:, :, :, 64 * j:64 * j + 64] = vt[:, :, :, 64 * t:64 * t + 64]
    nk = 64 * (len(tiles) - 1) + min(64, N - 64 * tiles[-1])            # the logical key count: the last listed tile may be ragged
    out = torch.zeros(B, N, H * 64, device=qp.device, dtype=BF)
    ops.attn_fwd(qp, kg, vg, out, N, nk, SCALE)
    assert _last_kernel() == "ld_attn_q64_kernel"
    return out


@pytest.mark.parametrize("N,P,G,w,B,H", [(1890, 90, 200, 0, 1, 1), (1890, 90, 200, 1, 2, 3), (2000, 100, 190, 1, 1, 1), (1000, 0, 125, 1, 1, 2),
                                         (2048, 128, 320, 1, 1, 1)])
def test_bit_identity_with_the_dense_kernel_on_gathered_tiles(cuda, N, P, G, w, B, H):
    """Check 2: per query block, the same bits as ld_attn_q64_kernel on the block's tiles made contiguous."""
    qp, kp, vt = _packed(*_randn(cuda, B, H, N, seed=N + 7))
    out = _window(qp, kp, vt, N, P, G, w)
    for b, tiles in enumerate(rule(N, P, G, w)):
        ref = _gathered_dense(qp, kp, vt, N, tiles)
        rows = slice(256 * b, min(256 * b + 256, N))
        assert torch.equal(out[:, rows], ref[:, rows]), f"block {b}"


@pytest.mark.parametrize("N,P,G", [(1890, 90, 200), (1000, 0, 125), (2048, 128, 320)])
def test_window_covering_all_frames_is_the_dense_launch(cuda, N, P, G):
    """Check 3."""
    from landiff_amd import ops
    qp, kp, vt = _packed(*_randn(cuda, 1, 2, N, seed=N + 3))
    ref = torch.zeros(1, N, 128, device=cuda, dtype=BF)
    ops.attn_fwd(qp, kp, vt, ref, N, N, SCALE)
    assert _last_kernel() == "ld_attn_q64_kernel"
    frames = -(-(N - P) // G)
    for w in (frames - 1, frames, 10 ** 6):
        assert torch.equal(_window(qp, kp, vt, N, P, G, w), ref), w


@pytest.mark.parametrize("N,P,G,w", CASES)
def test_random_data_against_fp32_softmax(cuda, N, P, G, w):
    """Check 4: N(0, 1) inputs, the bound of tests/test_gpu_attn.py for this kernel; two launches give the same bits."""
    q, k, v = _randn(cuda, 2, 2, N, seed=N + 11 + w)
    qp, kp, vt = _packed(q, k, v)
    out = _window(qp, kp, vt, N, P, G, w)
    err = (out.float() - _reference(q, k, v, N, P, G, w)).abs().max().item()
    print(f"window N={N} P={P} G={G} w={w}: max abs err {err:.3e}")
    assert err < 2e-2
    assert torch.equal(_window(qp, kp, vt, N, P, G, w), out)


def _spike_error(out, ref):
    return (out.float() - ref).abs().max().item() / ref.abs().max().item()


def test_overflow_falls_back_to_the_safe_pass(cuda):
    """Check 5: the spiked input of test_attn_pipelined_overflow_falls_back and its bound (relative error < 0.2) against the masked
    reference: denominators overflow the fast pass, the block redoes its own tile list with the running-max pass."""
    N, P, G, w = 1890, 90, 200, 1
    q, k, v = _randn(cuda, 1, 2, N, seed=0, q_scale=6.0, spike=True)
    out = _window(*_packed(q, k, v), N, P, G, w)
    err = _spike_error(out, _reference(q, k, v, N, P, G, w))
    print(f"window overflow fallback: relative err {err:.3e}")
    assert err == err and err < 0.2


@pytest.mark.parametrize("N,P,G,w", CASES)
def test_forced_safe_pass_walks_the_same_tiles(cuda, monkeypatch, N, P, G, w):
    """Check 5: LD_ATTN_SAFE=1 (re-read per call under LD_TUNING=1) runs the running-max pass over the same tile lists."""
    q, k, v = _randn(cuda, 1, 2, N, seed=N + 13)
    monkeypatch.setenv("LD_ATTN_SAFE", "1")
    out = _window(*_packed(q, k, v), N, P, G, w, expect="ld_attn_q64_win_kernel[safe pass forced]")
    monkeypatch.delenv("LD_ATTN_SAFE")
    err = (out.float() - _reference(q, k, v, N, P, G, w)).abs().max().item()
    print(f"window safe pass N={N} w={w}: max abs err {err:.3e}")
    assert err < 2e-2


def test_dynamic_form(cuda, monkeypatch):
    """Check 6 (and the fallback count of check 5): the smallest grid that takes the dynamic form on 256 CUs."""
    from landiff_amd import ops
    B, H, N, P, G, w = 4, 64, 2048, 128, 240, 1
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert B * H * ((N + 255) // 256) >= 4 * 2 * cus, "the grid does not reach the dynamic form on this device"
    q, k, v = _randn(cuda, B, H, N, seed=21)
    qp, kp, vt = _packed(q, k, v)
    monkeypatch.setenv("LD_ATTN_DYN", "0")
    ref = _window(qp, kp, vt, N, P, G, w).clone()
    monkeypatch.delenv("LD_ATTN_DYN")
    err = (ref[:, :, :192].float() - _reference(q[:, :3], k[:, :3], v[:, :3], N, P, G, w)).abs().max().item()      # three heads of every batch
    assert err < 2e-2
    out = _window(qp, kp, vt, N, P, G, w, expect="ld_attn_q64_win_dyn_kernel")
    cnt = torch.full((1,), 7, device=cuda, dtype=torch.int32)
    ops.attn_last_fallbacks(cnt)
    assert torch.equal(out, ref) and cnt.item() == 0
    # two streams at once, each pulling through its own counter set
    q2, k2, v2 = _randn(cuda, B, H, N, seed=22)
    qp2, kp2, vt2 = _packed(q2, k2, v2)
    monkeypatch.setenv("LD_ATTN_DYN", "0")
    ref2 = _window(qp2, kp2, vt2, N, P, G, w).clone()
    monkeypatch.delenv("LD_ATTN_DYN")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    o1 = [_sentinel(cuda, B, N, H) for _ in range(3)]; o2 = [_sentinel(cuda, B, N, H) for _ in range(3)]
    torch.cuda.synchronize()
    for i in range(3):
        with torch.cuda.stream(s1):
            ops.attn_fwd_window(qp, kp, vt, o1[i][:, :N], N, SCALE, P, G, w)
            assert _last_kernel() == "ld_attn_q64_win_dyn_kernel"
        with torch.cuda.stream(s2):
            ops.attn_fwd_window(qp2, kp2, vt2, o2[i][:, :N], N, SCALE, P, G, w)
            assert _last_kernel() == "ld_attn_q64_win_dyn_kernel"
    torch.cuda.synchronize()
    for o, r in [(o, ref) for o in o1] + [(o, ref2) for o in o2]:
        _check_sentinel(o, N)
        assert torch.equal(o[:, :N], r)
    # a launch captured into a graph takes the static form: the same bits
    buf = _sentinel(cuda, B, N, H)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ops.attn_fwd_window(qp, kp, vt, buf[:, :N], N, SCALE, P, G, w)
            assert _last_kernel() == "ld_attn_q64_win_kernel"
        g.replay()
    torch.cuda.synchronize()
    _check_sentinel(buf, N)
    assert torch.equal(buf[:, :N], ref)
    # the fallback count word of the dynamic form: a spiked input leaves the window in the blocks that see the spike
    qs, ks, vs = _randn(cuda, B, H, N, seed=23, q_scale=6.0, spike=True)
    outs = _window(*_packed(qs, ks, vs), N, P, G, w, expect="ld_attn_q64_win_dyn_kernel")
    ops.attn_last_fallbacks(cnt)
    err = _spike_error(outs[:, :, :192], _reference(qs[:, :3], ks[:, :3], vs[:, :3], N, P, G, w))
    print(f"window dynamic: fallbacks {cnt.item()} of {B * H * 8} blocks, relative err {err:.3e}")
    assert cnt.item() > 0 and err == err and err < 0.2


# ---- runner: ControlDiTRunner(attn_window=...) at the DiTConfig.config0() shape ---------------------------------------------
@pytest.fixture(scope="module")
def cfg0(cuda):
    """config0 DiT (text 8, 8 frames of 1024 tokens, 129 key tiles, hidden 128) with seeded random weights, two sampler steps'
    inputs and the outputs of the runner without the option (computed once)."""
    from landiff_amd.config import DiTConfig
    from landiff_amd.weights import dit_spec, init_state
    d = DiTConfig.config0()
    assert (d.text_len, d.latent_frames, d.grid_h * d.grid_w, -(-d.seq_len // 64), d.hidden) == (8, 8, 1024, 129, 128)
    g = torch.Generator().manual_seed(31)
    shape = (1, d.latent_frames, d.in_channels, d.latent_h, d.latent_w)
    x0, dx = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    t = dict(d=d, main=init_state(dit_spec(d, False), 5), ctrl=init_state(dit_spec(d, True), 6),
             xs=[(x0 + 0.2 * s * dx).to(cuda) for s in range(2)], ts=[900, 500], scal=(-0.8, 0.6, 4.0),
             ctx=torch.randn(1, d.text_len, d.text_dim, generator=g),
             sem=(0.5 * torch.randn(d.latent_frames, d.in_channels, d.latent_h, d.latent_w, generator=g)).to(BF))
    t["dense"] = _steps(_runner(t, cuda), t)
    return t


def _runner(t, cuda, **kw):
    from landiff_amd.dit import ControlDiTRunner
    run = ControlDiTRunner(t["main"], t["ctrl"], t["d"], cuda, **kw)
    run.set_condition(t["ctx"], t["sem"])
    return run


def _steps(run, t, n=2):
    outs = []
    for s in range(n):
        out = torch.empty_like(t["xs"][s])
        run.step(t["xs"][s], t["ts"][s], *t["scal"], out)
        outs.append(out)
    torch.cuda.synchronize()
    return outs


def _spy(monkeypatch):
    """Wrap ops.attn_fwd_window: record the kernel of every call (and keep the last call's operands and output)."""
    from landiff_amd import ops
    real, seen = ops.attn_fwd_window, []

    def wrapper(q, k, vt, out, N, scale, prefix, group, window):
        r = real(q, k, vt, out, N, scale, prefix, group, window)
        seen.append(dict(kernel=_last_kernel(), args=(N, scale, prefix, group, window), q=q.clone(), k=k.clone(), vt=vt.clone(), out=out.clone()))
        return r
    monkeypatch.setattr(ops, "attn_fwd_window", wrapper)
    return seen


def test_runner_window_covering_all_frames_equals_the_dense_runner(cuda, cfg0, monkeypatch):
    seen = _spy(monkeypatch)
    for w in (7, 8):
        outs = _steps(_runner(cfg0, cuda, attn_window=w), cfg0)
        assert all(torch.equal(a, b) for a, b in zip(outs, cfg0["dense"])), w
    assert len(seen) == 2 * 2 * 3 and {s["kernel"] for s in seen} == {"ld_attn_q64_win_kernel"}


@pytest.mark.parametrize("fp8,overlap", [(False, "1"), (False, "0"), (True, "1"), ("mx", "1")])
def test_runner_window_kernel_runs_in_every_layer(cuda, cfg0, monkeypatch, fp8, overlap):
    """w = 1: every attention launch of both branches is the window kernel with the runner's (prefix, group, window) -- with the
    control / main overlap on and off and in both fp8 modes -- and one captured call satisfies the random-data check."""
    monkeypatch.setenv("LD_DIT_OVERLAP", overlap)
    seen = _spy(monkeypatch)
    d = cfg0["d"]
    run = _runner(cfg0, cuda, attn_window=1, fp8_gemm=fp8)
    assert run.overlap == (overlap == "1")
    outs = _steps(run, cfg0, n=1)
    assert torch.isfinite(outs[0]).all()
    assert len(seen) == d.layers_control + d.layers_main
    assert all(s["kernel"] == "ld_attn_q64_win_kernel" and s["args"] == (d.seq_len, 0.125, 8, 1024, 1) for s in seen)
    if fp8 is False and overlap == "1":
        assert not torch.equal(outs[0], cfg0["dense"][0])                     # the window changes the result
        c, N = seen[-1], d.seq_len
        q, k, v = c["q"][:, :, :N], c["k"][:, :, :N], c["vt"][:, :, :, :N].transpose(2, 3)
        err = (c["out"].float() - _reference(q, k, v, N, 8, 1024, 1)).abs().max().item()
        print(f"runner window call: max abs err {err:.3e}")
        assert err < 2e-2


def test_runner_dense_steps_and_the_step_counter(cuda, cfg0, monkeypatch):
    seen = _spy(monkeypatch)
    from landiff_amd.config import AttnWindowConfig
    run = _runner(cfg0, cuda, attn_window=AttnWindowConfig(frames=1, dense_steps=1))
    outs = _steps(run, cfg0)
    assert torch.equal(outs[0], cfg0["dense"][0]) and not torch.equal(outs[1], cfg0["dense"][1])
    assert len(seen) == 3                                                       # the second step's three layers
    run.set_condition(cfg0["ctx"], cfg0["sem"])                                 # a new video: the counter starts again
    again = _steps(run, cfg0)
    assert torch.equal(again[0], outs[0]) and torch.equal(again[1], outs[1]) and len(seen) == 6


def test_runner_window_composes_with_the_step_cache(cuda, cfg0, monkeypatch):
    """A computed step of the cached runner uses the window: threshold 0 computes every step, so the outputs are the windowed runner's."""
    from landiff_amd.dit_cache import StepCacheConfig
    want = _steps(_runner(cfg0, cuda, attn_window=1), cfg0)
    seen = _spy(monkeypatch)
    run = _runner(cfg0, cuda, attn_window=1, step_cache=StepCacheConfig(threshold=0.0), plan_timesteps=cfg0["ts"])
    outs = _steps(run, cfg0)
    assert [r["computed"] for r in run.cache_report] == [True, True]
    assert all(torch.equal(a, b) for a, b in zip(outs, want)) and len(seen) == 6


def test_runner_without_the_option_never_calls_the_window_form(cuda, cfg0, monkeypatch):
    seen = _spy(monkeypatch)
    outs = _steps(_runner(cfg0, cuda), cfg0)
    assert seen == [] and all(torch.equal(a, b) for a, b in zip(outs, cfg0["dense"]))


def test_runner_refuses_shapes_the_window_form_cannot_take(cuda):
    from landiff_amd.config import DiTConfig
    from landiff_amd.dit import ControlDiTRunner
    from landiff_amd.weights import dit_spec, init_state
    d = DiTConfig.tiny()
    with pytest.raises(ValueError, match="does not fit this DiT shape"):
        ControlDiTRunner(init_state(dit_spec(d, False), 1), init_state(dit_spec(d, True), 2), d, cuda, attn_window=1)
    with pytest.raises(ValueError, match="attn_exact"):
        ControlDiTRunner({}, {}, DiTConfig.config0(), cuda, attn_exact=True, attn_window=1)
