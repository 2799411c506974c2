"""The input of the workgroup-vote tests: one query row whose max-free fast pass overflows, in the last wave that stores rows of
the last query block -- every other row of its workgroup stays inside the fast pass's window, so the workgroup takes the
running-max pass only if that one wave's flag reaches all the others (attn_window_vote, csrc/ld_attn_dev.h).

N = 1122 (Npad 1152): the last workgroup starts at row 1024 for every tile (256 rows: ld_attn_q64 and the 8-wave ld_attn_p16; 128
rows: the 4-wave ld_attn_p16).  Row 1121 is the last row: wave 1 of 4 (64-row waves), wave 3 of 4 and wave 3 of 8 (32-row waves); the
waves behind it hold no stored row.  Shared by tests/test_attn_route_host.py (what the seed gives, on the CPU) and
tests/test_gpu_variants.py (the kernels)."""
import torch

B, H, N, ROW, Q_GAIN, SEED = 1, 2, 1122, 1121, 40.0, 6
SCALE = 0.125
LOG2E = 1.4426950408889634


def inputs():
    """bf16 q, k, v [B, H, N, 64] on the CPU; row ROW of q (every head) scaled by Q_GAIN before rounding."""
    g = torch.Generator(device="cpu").manual_seed(SEED)
    q = torch.randn(B, H, N, 64, generator=g)
    k = torch.randn(B, H, N, 64, generator=g)
    v = torch.randn(B, H, N, 64, generator=g)
    q[:, :, ROW] *= Q_GAIN
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def reference(q, k, v):
    """torch fp32 softmax attention of the bf16 inputs -> [B, N, H * 64]"""
    s = (q.float() @ k.float().transpose(-1, -2)) * SCALE
    return (torch.softmax(s, -1) @ v.float()).permute(0, 2, 1, 3).reshape(q.shape[0], q.shape[2], -1)


def log2_scores(q, k):
    """the exponents the fast pass feeds to exp2: [B, H, N, N]"""
    return (q.float() @ k.float().transpose(-1, -2)) * (SCALE * LOG2E)
