"""ops.attn_mask_tables (the one builder of the masked attention kernel's four label arrays) and the host-side guards of
ops.attn_fwd; the arithmetic premise of the count design of tests/test_gpu_attn_masked.py."""
import numpy as np
import pytest
import torch

from landiff_amd import ops
from landiff_amd.config import TokenizerConfig
from landiff_amd.detokenizer import decoder_frame_ids
from landiff_amd.tokenizer_encoder import encoder_attention_labels, encoder_padded_len

INF = np.iinfo(np.int32).max


def _by_hand(fid_q, fid_k, Npad):
    """The arrays as the two stage modules built them before the builder existed."""
    fq = np.zeros(Npad, np.int32); fq[:len(fid_q)] = fid_q
    fk = np.full(Npad, INF, np.int32); fk[:len(fid_k)] = fid_k
    kt = fk.reshape(-1, 64)
    return fq, fk, kt.min(1), kt.max(1)


@pytest.mark.parametrize("cfg", [TokenizerConfig.tiny(), TokenizerConfig.config0(), TokenizerConfig()], ids=["tiny", "config0", "full"])
def test_tables_equal_the_hand_built_arrays(cfg):
    fid = decoder_frame_ids(cfg)
    N = cfg.seq_len
    cases = [(fid, fid, (N + 127) // 128 * 128)]
    qv, kv, ql, kl = encoder_attention_labels(cfg)
    Npad = encoder_padded_len(cfg)
    assert Npad % 128 == 0 and Npad >= cfg.n_visual + (N - cfg.n_visual + 127) // 128 * 128
    cases += [(qv, kv, Npad), (ql, kl, Npad)]
    for fq, fk, npad in cases:
        got = ops.attn_mask_tables(fq, fk, npad)
        for g, w in zip(got, _by_hand(fq, fk, npad)):
            assert g.dtype == torch.int32 and g.is_contiguous() and np.array_equal(g.numpy(), w)


def test_tables_padding_and_tile_ranges():
    fq, fk, kmin, kmax = ops.attn_mask_tables([3, -1, 2], np.arange(70)[::-1], 128)
    assert fq.tolist() == [3, -1, 2] + [0] * 125
    assert fk[:70].tolist() == list(range(69, -1, -1)) and (fk[70:] == INF).all()
    assert kmin.tolist() == [6, 0] and kmax.tolist() == [69, INF]


def test_unmasked_row_offset_is_refused_before_anything_else():
    """q_row0 without a mask on >= 6 key tiles: ValueError ahead of every other check (no library, no device needed)."""
    t = torch.zeros(1)
    with pytest.raises(ValueError, match="q_row0"):
        ops.attn_fwd(t, t, t, t, 64, 6 * 64 - 63, 0.125, q_row0=128)
    with pytest.raises(ValueError, match="q_row0"):
        ops.attn_fwd(t, t, t, t, 64, 4096, 0.125, q_row0=2, exact=True)


def test_count_design_decodes_exactly():
    """out = bf16(fp32(count) * fp32(1 / total)) decodes to `count` by round(out * total) for every count < 64 and every total up to
    18 768 (count <= total), also with the reciprocal one fp32 ulp off either way."""
    total = torch.arange(1, 18769, dtype=torch.float32)[:, None]
    count = torch.arange(0, 64, dtype=torch.float32)[None, :]
    inv = 1.0 / total
    for r in (inv, torch.nextafter(inv, torch.zeros_like(inv)), torch.nextafter(inv, torch.full_like(inv, 2.0))):
        out = (count * r).to(torch.bfloat16).double()
        ok = (torch.round(out * total.double()) == count.double()) | (count > total)
        assert bool(ok.all())
