"""The label-masked attention kernel (ld_attn_kernel in ld_attn.hip: ld_attn_fwd_bf16 with fid_q / fid_k), element by element.

The kernel decides per 128-row block which key tiles to stage (kt_min[t] <= the block's largest query label), per 32-row wave
which staged tiles to skip (tile min > the wave's largest label) and which need the element mask (tile max > the wave's smallest
label); query labels past Nq are clamped, a first-valid-key flag interacts with the deferred rescale, and the loop runs two
stages per trip while jumping over unneeded ones.  Every case asserts that this kernel ran, writes into a buffer of NaN sentinels
(the rows outside [q_row0, q_row0 + Nq), three rows behind the last one) that must come back untouched, and uses the product's
own table builder (ops.attn_mask_tables).  Two data designs on every layout:

  * count: Q = 0, so every score is 0 and every visible key has p = 1 exactly; V is the one-hot of class(k) = k % 64, so
    out[q][d] = count_d(q) / total(q) with exact integer sums in fp32 -- the only roundings are 1 / total, one fp32 multiply and
    the bf16 store, 2^-8 relative at most.  For count_d < 64 (asserted) round(out * total) recovers count_d, so ONE key leaked
    or dropped anywhere changes an integer;
  * random: N(0, 1) q, k, v (and q x 4: running-max rebases) against a float64 softmax over the dense mask, computed from the
    kernel's own bf16(q * scale * log2 e).  Per-element bound (2^-8 + delta) (A + |ref|), A = the softmax-weighted mean of |v|:
    half a bf16 ulp on every P that enters P V (the denominator sums unrounded P), half an ulp on the stored output, and delta =
    2^-23 (visible keys + 64 max_k sum_d |q_d k_d| + 16) for the fp32 steps -- two sums of at most `visible` positive terms
    (n 2^-24 each in any order), the 64-term score accumulation whose error enters 2^s on both sides of the quotient, and
    exp2 / the rescale multiplies / the reciprocal at a few ulps.  Rows with one visible key return its V row bit for bit, rows
    with none exact zeros; two launches give the same bits.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN16 = 0x7FA5                      # sentinel bit pattern (a quiet bf16 NaN)
EXTRA_ROWS = 3                      # sentinel rows behind row N of every batch: o_batch_stride != N * o_row_stride
SCALE = 0.125
Launch = namedtuple("Launch", "fq fk row0 nq")        # labels indexed by absolute row / key, query rows [row0, row0 + nq)
Layout = namedtuple("Layout", "B H N Npad launches")
CHECKED = {"count_integers": 0}


def _last_kernel():
    from landiff_amd import _lib
    return (_lib.load().ld_attn_last_kernel() or b"").decode()


def _decoder(T, tpf, nI, nP, B=1, H=2):
    from landiff_amd.config import TokenizerConfig
    from landiff_amd.detokenizer import decoder_frame_ids
    cfg = TokenizerConfig(grid_h=1, grid_w=tpf, temporal=T, pframe_tokens=nP, num_latent_tokens=nI + (T - 1) * nP)
    fid = decoder_frame_ids(cfg)
    N = len(fid)
    assert N == T * tpf + nI + (T - 1) * nP
    return Layout(B, H, N, (N + 127) // 128 * 128, [Launch(fid, fid, 0, N)])


def _encoder(cfg, H=2):
    """The two launches of TokenizerEncoder.encode_rows: visual rows, then latent rows at q_row0 = n_visual, one att buffer."""
    from landiff_amd.tokenizer_encoder import encoder_attention_labels, encoder_padded_len
    qv, kv, ql, kl = encoder_attention_labels(cfg)
    N, nv = cfg.seq_len, cfg.n_visual
    return Layout(1, H, N, encoder_padded_len(cfg), [Launch(qv, kv, 0, nv), Launch(ql, kl, nv, N - nv)])


def _encoder_small(tpf, T, nI, nP):
    from landiff_amd.config import TokenizerConfig
    return _encoder(TokenizerConfig(grid_h=1, grid_w=tpf, temporal=T, pframe_tokens=nP, num_latent_tokens=nI + (T - 1) * nP))


def _adversarial(kind):
    N, Npad = 700, 768                                   # 11 key tiles, the last one ragged (60 keys); 6 query blocks
    rng = np.random.RandomState(11)
    ar = np.arange(N)
    if kind == "equal":
        fq = fk = np.zeros(N, np.int64)
    elif kind == "descending":
        # key k carries N-1-k, query q carries N-1-q-20: q sees the keys k >= q + 20.  Blocks 1.. do not need stage 0; a wave at rows
        # 64 t + 32 .. 64 t + 63 starts at tile t, which is fully masked for its lanes past row 64 t + 43 only; rows 680.. see no
        # key, row 679 exactly key N - 1 in the ragged tile
        fk = N - 1 - ar
        fq = N - 1 - ar - 20
    elif kind == "iid":
        fq = fk = rng.randint(0, 5, N)
    elif kind == "gaps":
        # the first query block needs exactly the key tiles {0, 2, 3, 6, 10}: runs of 1, 2 and 3 skipped stages, a needed tile
        # behind an odd and behind an even run; the other blocks see everything
        need = np.isin(ar // 64, [0, 2, 3, 6, 10])
        fk = np.where(need, 0, 1)
        fq = np.where(ar < 128, 0, 1)
    elif kind == "independent":
        # key N - 1 alone carries the smallest key label 0: queries of label 0 see exactly that key, queries of label -1 none;
        # the whole block of rows 256 .. 383 carries -1 (it stages nothing)
        fk = rng.randint(1, 10, N); fk[N - 1] = 0
        fq = rng.randint(0, 10, N)
        fq[rng.choice(N, 40, replace=False)] = -1
        fq[256:384] = -1
        fq[[0, 31, 200, 639, 640, 699]] = 0
    else:
        raise KeyError(kind)
    return Layout(1, 2, N, Npad, [Launch(fq.astype(np.int32), fk.astype(np.int32), 0, N)])


@functools.lru_cache(maxsize=None)
def _layout(name):
    if name == "dec500":            # frames straddle tiles and waves
        return _decoder(5, 90, 22, 7)
    if name == "dec512":            # N = Npad, every label boundary on a tile and block boundary: no element mask, no padding tile
        return _decoder(3, 128, 64, 32)
    if name == "dec500_b2h3":       # the label arrays are shared across batch and head
        return _decoder(5, 90, 22, 7, B=2, H=3)
    if name == "enc_mid":           # the "mid" config of test_gpu_tokenizer_encoder.py: nv = 264, N = 372, Npad = 512
        return _encoder_small(66, 4, 45, 21)
    if name == "enc_256":           # q_row0 = 256, a multiple of the query block; N = 312
        return _encoder_small(64, 4, 20, 12)
    return _adversarial(name)


LAYOUTS = ["dec500", "dec512", "enc_mid", "enc_256", "equal", "descending", "iid", "gaps", "independent", "dec500_b2h3"]


def test_layouts_are_what_the_cases_claim():
    """The layouts' own premises (host arithmetic only)."""
    assert (_layout("dec500").N, _layout("dec512").N, _layout("dec512").Npad) == (500, 512, 512)
    m, e = _layout("enc_mid"), _layout("enc_256")
    assert (m.launches[1].row0, m.N, m.Npad) == (264, 372, 512) and (e.launches[1].row0, e.N) == (256, 312)
    kl = m.launches[1].fk
    assert (np.diff(kl.astype(np.int64)) < 0).any(), "the latent launch's key labels are not monotone in key order"
    g = _layout("gaps").launches[0]
    ktmin = g.fk[:640].reshape(-1, 64).min(1).tolist() + [int(g.fk[640:].min())]
    assert [t for t in range(11) if ktmin[t] <= g.fq[:128].max()] == [0, 2, 3, 6, 10]
    assert all(ktmin[t] <= g.fq[128:].max() for t in range(11))
    for name in ("descending", "independent"):
        L = _layout(name).launches[0]
        vis = (L.fk[None, :].astype(np.int64) <= L.fq[:, None]).sum(1)
        assert (vis == 0).sum() >= 20 and (vis == 1).sum() >= 1, name
    L = _layout("independent").launches[0]
    assert (L.fq[256:384] == -1).all() and L.fk.min() == 0 and L.fk[699] == 0 and (L.fk[:699] > 0).all()
    d = _layout("descending").launches[0]
    assert d.fq[128:256].max() < d.fk[:128].min() and d.fq[128:256].max() >= d.fk[128:192].min()       # block 1 starts at stage 2


def _dense_mask(L, N, dev, rows=None):
    """allowed[q, kv] of a launch from its labels: the one restatement of the mask the references use (bool [rows, N])."""
    fq = torch.from_numpy(np.asarray(L.fq, np.int64)).to(dev)
    fk = torch.from_numpy(np.asarray(L.fk, np.int64)).to(dev)[:N]
    if rows is None:
        rows = torch.arange(L.row0, L.row0 + L.nq, device=dev)
    return fk[None, :] <= fq[rows][:, None]


def _sentinel_out(lay, dev):
    bits = torch.full((lay.B, lay.N + EXTRA_ROWS, lay.H * 64), NAN16, device=dev, dtype=torch.int16)
    return bits, bits.view(BF)[:, :lay.N]


def _launch(lay, which, q, k, vt, out, exact=False):
    from landiff_amd import ops
    for i in which:
        L = lay.launches[i]
        ops.attn_fwd(q, k, vt, out, L.nq, lay.N, SCALE, *_tables(lay, i, q.device), q_row0=L.row0, exact=exact)
        assert _last_kernel().startswith("ld_attn_kernel"), _last_kernel()


def _tables(lay, i, dev):
    """The four mask arrays of launch i, from the product's builder."""
    from landiff_amd import ops
    L = lay.launches[i]
    tabs = ops.attn_mask_tables(L.fq, L.fk, lay.Npad, dev)
    fq, fk, kmin, kmax = tabs
    assert all(t.dtype == torch.int32 and t.is_cuda for t in tabs)
    assert fq.numel() == fk.numel() == lay.Npad and kmin.numel() == kmax.numel() == lay.Npad // 64
    return tabs


def _check_written(lay, which, bits):
    """Rows outside the launched ranges keep the sentinel; no row inside is NaN."""
    written = torch.zeros(lay.N + EXTRA_ROWS, dtype=torch.bool, device=bits.device)
    for i in which:
        L = lay.launches[i]
        written[L.row0:L.row0 + L.nq] = True
    assert bool((bits[:, ~written] == NAN16).all()), "a store outside [q_row0, q_row0 + Nq)"
    assert not bool(torch.isnan(bits.view(BF)[:, written]).any()), "a NaN (or an unwritten element) inside the launched rows"


def _rows_of(out, L, H):
    return out[:, L.row0:L.row0 + L.nq].reshape(out.shape[0], L.nq, H, 64).permute(0, 2, 1, 3)        # [B, H, nq, 64]


# ---- (a) count design ----------------------------------------------------------------------------------------------------------
def _count_operands(lay, dev, cls):
    g = torch.Generator(device=dev).manual_seed(lay.N)
    q = torch.zeros(lay.B, lay.H, lay.Npad, 64, device=dev, dtype=BF)
    k = torch.zeros_like(q)
    k[:, :, :lay.N] = torch.randn(lay.B, lay.H, lay.N, 64, device=dev, generator=g).to(BF)
    onehot = torch.nn.functional.one_hot(cls, 64)                                   # [N, 64]
    vt = torch.zeros(lay.B, lay.H, 64, lay.Npad, device=dev, dtype=BF)
    vt[:, :, :, :lay.N] = onehot.t().to(BF)
    return q, k, vt, onehot


def _check_counts_small(lay, which, out, onehot, tally):
    for i in which:
        L = lay.launches[i]
        mask = _dense_mask(L, lay.N, out.device)
        counts = mask.double() @ onehot.double()                                    # [nq, 64], exact integers
        total = mask.sum(1).double()
        assert counts.max().item() < 64 and total.max().item() <= 18768, "premise of the exact decoding"
        got = _rows_of(out, L, lay.H).double()                                      # [B, H, nq, 64]
        decoded = torch.round(got * total[:, None])
        bad = decoded != counts
        assert not bool(bad.any()), (f"launch {i}: {int(bad.sum())} (row, class) counts differ, first at (b, h, row, class) "
                                     f"{tuple(bad.nonzero()[0].tolist())}: {decoded[bad][0].item()} for {counts.expand_as(bad)[bad][0].item()}")
        assert bool((got[:, :, total == 0] == 0).all()), "a row with no visible key is not exact zeros"
        if tally:
            CHECKED["count_integers"] += got.numel()


@pytest.mark.parametrize("name", LAYOUTS)
def test_masked_count(cuda, name):
    """Exact membership: every (row, class) count of visible keys decoded from the output equals the dense mask's."""
    lay = _layout(name)
    assert lay.N < 4096
    cls = torch.arange(lay.N, device=cuda) % 64
    q, k, vt, onehot = _count_operands(lay, cuda, cls)
    every = list(range(len(lay.launches)))
    plans = [every] if len(every) == 1 else [[0], [1], every]          # each launch alone first: the other group's rows untouched
    for which in plans:
        bits, out = _sentinel_out(lay, cuda)
        _launch(lay, which, q, k, vt, out)
        _check_written(lay, which, bits)
        _check_counts_small(lay, which, out, onehot, tally=which == every)      # (the single-launch runs repeat the same integers)
    print(f"\n{name}: {CHECKED['count_integers']} (row, class) integers checked so far in this file")


# ---- (b) random design ---------------------------------------------------------------------------------------------------------
def _random_operands(lay, dev, q_scale, seed):
    """Q rows in [N, Npad) hold live data too (the kernel computes them and must not store them); K and V^T padding is zero."""
    g = torch.Generator(device=dev).manual_seed(seed)
    q = (torch.randn(lay.B, lay.H, lay.Npad, 64, device=dev, generator=g) * q_scale).to(BF)
    k = torch.zeros_like(q)
    k[:, :, :lay.N] = torch.randn(lay.B, lay.H, lay.N, 64, device=dev, generator=g).to(BF)
    vt = torch.zeros(lay.B, lay.H, 64, lay.Npad, device=dev, dtype=BF)
    vt[:, :, :, :lay.N] = torch.randn(lay.B, lay.H, 64, lay.N, device=dev, generator=g).to(BF)
    return q, k, vt


def _reference(q, k, vt, N, rows, mask):
    """float64 softmax over the dense mask for query rows `rows` of every (b, h): (ref, bound) [B, H, len(rows), 64]."""
    c = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)   # the launcher's fp32 product
    qs = (q[:, :, rows].float() * c.to(q.device)).to(BF).double()                   # the kernel's one extra rounding of q
    kd, vd = k[:, :, :N].double(), vt[:, :, :, :N].double().transpose(-1, -2)
    s = (qs @ kd.transpose(-1, -2)).masked_fill(~mask, float("-inf"))               # log2 units
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))      # rows with no visible key: all 0
    den = p.sum(-1, keepdim=True)
    safe = den.clamp(min=1e-300)
    ref, A = (p @ vd) / safe, (p @ vd.abs()) / safe
    sabs = (qs.abs() @ kd.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    delta = 2.0 ** -23 * (mask.sum(-1, keepdim=True).double() + 64 * sabs + 16)
    return ref, (2.0 ** -8 + delta) * (A + ref.abs())


def _check_random(lay, i, q, k, vt, out, tag):
    L = lay.launches[i]
    mask = _dense_mask(L, lay.N, out.device)
    rows = torch.arange(L.row0, L.row0 + L.nq, device=out.device)
    ref, bound = _reference(q, k, vt, lay.N, rows, mask)
    got16 = _rows_of(out, L, lay.H)
    got = got16.double()
    d = (got - ref).abs()
    vis = mask.sum(1)
    assert bool((got[:, :, vis == 0] == 0).all()), "a row with no visible key is not exact zeros"
    one = (vis == 1).nonzero().flatten()
    if one.numel():
        keys = mask[one].int().argmax(1)
        want = vt[:, :, :, keys].transpose(-1, -2)                                  # [B, H, n, 64]: that key's V row
        assert torch.equal(got16[:, :, one], want), "a row with one visible key is not that key's V row bit for bit"
    live = bound > 0
    frac = (d[live] / bound[live]).max().item() if bool(live.any()) else 0.0
    print(f"\n{tag} launch {i}: worst {frac:.3f} of the per-element bound; rows with no / one visible key: "
          f"{int((vis == 0).sum())} / {one.numel()}")
    over = d > bound
    assert not bool(over.any()), (f"{int(over.sum())} elements over their bound, worst at (b, h, row, d) "
                                  f"{np.unravel_index((d - bound).flatten().argmax().item(), tuple(d.shape))}: {frac:.3f} of it")


@pytest.mark.parametrize("q_scale", [1.0, 4.0])
@pytest.mark.parametrize("name", LAYOUTS)
def test_masked_random(cuda, name, q_scale):
    """Numerics: every element within its derived bound of the float64 reference; two launches give the same bits."""
    lay = _layout(name)
    q, k, vt = _random_operands(lay, cuda, q_scale, seed=lay.N + int(q_scale))
    every = list(range(len(lay.launches)))
    plans = [every] if len(every) == 1 else [[0], [1], every]
    for which in plans:
        bits, out = _sentinel_out(lay, cuda)
        _launch(lay, which, q, k, vt, out)
        _check_written(lay, which, bits)
        for i in which:
            _check_random(lay, i, q, k, vt, out, f"{name} q x {q_scale:g}")
    bits2, again = _sentinel_out(lay, cuda)
    _launch(lay, every, q, k, vt, again)
    assert torch.equal(bits2, bits), "two launches differ"


def test_masked_exact_entry_point_runs_the_same_kernel(cuda):
    """Masked problems take the plain kernel in ld_attn_fwd_bf16_exact too (_launch asserts the kernel): equal bits."""
    lay = _layout("dec500")
    q, k, vt = _random_operands(lay, cuda, 4.0, seed=9)
    bits, out = _sentinel_out(lay, cuda)
    _launch(lay, [0], q, k, vt, out)
    bits_x, out_x = _sentinel_out(lay, cuda)
    _launch(lay, [0], q, k, vt, out_x, exact=True)
    _check_written(lay, [0], bits_x)
    assert torch.equal(bits, bits_x)


def test_unmasked_row_offset_on_pipelined_shapes_is_refused(cuda):
    """q_row0 without a mask on >= 6 key tiles would take a pipelined kernel, whose 256-row blocks read Q past the offset block:
    the wrapper raises before any launch (nothing is launched here either); masked and short problems keep the offset."""
    from landiff_amd import ops
    lay = _layout("enc_mid")
    q, k, vt = _random_operands(lay, cuda, 1.0, seed=1)
    bits, out = _sentinel_out(lay, cuda)
    L = lay.launches[1]
    before = _last_kernel()
    with pytest.raises(ValueError, match="q_row0"):
        ops.attn_fwd(q, k, vt, out, L.nq, 6 * 64 - 63, SCALE, q_row0=L.row0)
    with pytest.raises(ValueError, match="q_row0"):
        ops.attn_fwd(q, k, vt, out, L.nq, lay.N, SCALE, q_row0=L.row0, exact=True)
    torch.cuda.synchronize()
    assert bool((bits == NAN16).all()) and _last_kernel() == before
    # five key tiles, unmasked, offset: the plain kernel, rows [row0, row0 + nq) only
    Nk = 5 * 64
    ops.attn_fwd(q, k, vt, out, L.nq, Nk, SCALE, q_row0=L.row0)
    assert _last_kernel().startswith("ld_attn_kernel")
    _check_written(lay, [1], bits)
    rows = torch.arange(L.row0, L.row0 + L.nq, device=cuda)
    ref, bound = _reference(q, k, vt, Nk, rows, torch.ones(L.nq, Nk, dtype=torch.bool, device=cuda))
    assert bool(((_rows_of(out, L, lay.H).double() - ref).abs() <= bound).all())


# ---- full shape ----------------------------------------------------------------------------------------------------------------
def test_masked_full_shape_encoder_two_launches(cuda):
    """TokenizerConfig() encoder labels (N = 18 768, nv = 17 550, H = 2), both launches into one buffer.  Count design over ALL
    rows with class(k) = (k // 64) % 64 (counts of about 300): |out * total - count_d| <= 0.5 + count_d 2^-8 (half a bf16 ulp
    of the stored quotient is at most 2^-8 relative), i.e. under 2 keys -- a lost or extra half tile (32 keys) or a wrong row
    offset fails, ONE key does not: single keys are the small layouts' job.  Random design on spot rows against float64 with the
    small layouts' bound: first / last rows, frame boundaries, the last visual row (inside a block whose other rows are latent),
    the first latent rows around a block boundary, the first and last P latent of a middle frame."""
    from landiff_amd.config import TokenizerConfig
    cfg = TokenizerConfig()
    lay = _encoder(cfg)
    N, nv = lay.N, cfg.n_visual
    assert (N, nv, lay.Npad) == (18768, 17550, 18944)
    # count design
    cls = (torch.arange(N, device=cuda) // 64) % 64
    q, k, vt, onehot = _count_operands(lay, cuda, cls)
    bits, out = _sentinel_out(lay, cuda)
    _launch(lay, [0, 1], q, k, vt, out)
    _check_written(lay, [0, 1], bits)
    onehot32 = onehot.float()
    worst = 0.0
    for L in lay.launches:
        for r0 in range(L.row0, L.row0 + L.nq, 2048):
            rows = torch.arange(r0, min(r0 + 2048, L.row0 + L.nq), device=cuda)
            mask = _dense_mask(L, N, cuda, rows)
            counts = (mask.float() @ onehot32).double()                             # integers below 2^24: exact in fp32
            total = mask.sum(1).double()
            assert total.min().item() > 0
            got = out[0, rows].reshape(len(rows), lay.H, 64).permute(1, 0, 2).double()
            err = (got * total[:, None] - counts).abs()
            tol = 0.5 + counts * 2.0 ** -8
            worst = max(worst, (err / tol).max().item())
            assert bool((err <= tol).all()), (f"rows {r0}..: {int((err > tol).sum())} (row, class) counts off, worst "
                                              f"{err.max().item():.2f} keys")
            CHECKED["count_integers"] += got.numel()
    print(f"\nfull shape: count design worst {worst:.3f} of its tolerance; {CHECKED['count_integers']} (row, class) values "
          "checked so far in this file")
    # random design, spot rows
    nI, nP = cfg.iframe_tokens, cfg.pframe_tokens
    p0 = nv + nI + 5 * nP                                                           # first P latent of frame 6
    spots = {0: [0, 1349, 1350, nv - 1], 1: [nv, nv + 127, nv + 128, p0, p0 + nP - 1, N - 1]}
    for q_scale in (1.0, 4.0):
        q, k, vt = _random_operands(lay, cuda, q_scale, seed=40 + int(q_scale))
        bits, out = _sentinel_out(lay, cuda)
        _launch(lay, [0, 1], q, k, vt, out)
        _check_written(lay, [0, 1], bits)
        for i, rows_l in spots.items():
            rows = torch.tensor(rows_l, device=cuda)
            ref, bound = _reference(q, k, vt, N, rows, _dense_mask(lay.launches[i], N, cuda, rows))
            got = out[:, rows].reshape(1, len(rows_l), lay.H, 64).permute(0, 2, 1, 3).double()
            d = (got - ref).abs()
            print(f"full shape q x {q_scale:g} launch {i}: worst {(d / bound).max().item():.3f} of the per-element bound")
            assert bool((d <= bound).all()), (d / bound).amax(dim=(0, 1, 3)).tolist()
