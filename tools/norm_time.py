"""The norm family (ld_norm_*.hip) and the other MXFP8 producers at DiT size: output hashes and device-event times, for one build of
the library or several side by side -- the same seeded inputs for each, timed in turn within every repetition.
usage: python tools/norm_time.py [--small] [--only SUBSTR] [--reps N] [lib.so ...]       (no library: the shipped one)
Two copies of one build among the libraries give the spread that a difference between two builds has to exceed.  LD_LN_FAST /
LD_GN_ROWS from the environment apply to every library (a build that reads them once per process cannot switch later)."""
import os, sys, statistics
os.environ.setdefault("LD_TUNING", "1")
sys.path.insert(0, ".")
import torch
from landiff_amd import _lib, ops

args = sys.argv[1:]
small = "--small" in args
only = args[args.index("--only") + 1] if "--only" in args else ""
reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 20
paths = [a for i, a in enumerate(args) if a.endswith(".so") and (i == 0 or args[i - 1] not in ("--only", "--reps"))] or [_lib.LIB_PATH]
libs = []
for path in paths:                       # one binding per file; ops.* calls whichever _lib._lib names
    _lib._lib, _lib.LIB_PATH = None, path
    libs.append(_lib.load())
dev, BF = torch.device("cuda:0"), torch.bfloat16
g = torch.Generator().manual_seed(11)
rnd = lambda *s, scale=1.0: (scale * torch.randn(*s, generator=g)).to(dev)

# DiT size: rows 35552 = B 2 x N 17776 (226 text rows each), D 1920; --small: the shapes of the tests
B, N, T, D, H = (2, 70, 13, 256, 3) if small else (2, 17776, 226, 1920, 30)
rows, Npad = B * N, -(-N // 64) * 64
x, xf = rnd(rows, D).to(BF), rnd(rows, D)
w, b = (1 + 0.1 * rnd(D)).to(BF), (0.1 * rnd(D)).to(BF)
ada = rnd(B, 12 * D, scale=0.3).to(BF)
mod = dict(mod=ada, mod_bstride=12 * D, shift_img=0, scale_img=D, shift_txt=6 * D, scale_txt=7 * D, rows_per_batch=N, text_len=T)
x4 = rnd(rows, 4 * D).to(BF)
w1, b1 = rnd(4 * D, D, scale=D ** -0.5).to(BF), rnd(4 * D).to(BF)
qkv = rnd(rows, 3 * H * 64).to(BF)
qk_ln = tuple((1 + 0.1 * rnd(64)).to(BF) if i % 2 == 0 else (0.1 * rnd(64)).to(BF) for i in range(4))
ang = torch.rand(N, 32, generator=g) * 6.2831853
rope = (torch.cos(ang).to(dev), torch.sin(ang).to(dev))
# GroupNorm: C 128 takes the rows kernel, C 24 (3 chunks do not divide 256) the flat one; zq at half resolution
Fg, Tg, Hg, Wg = (2, 3, 6, 12) if small else (1, 5, 120, 180)
gn = {}
for C, G in ((128, 32), (24, 3)):
    gx = (rnd(Fg * Tg, Hg, Wg, C) * 1.5 + 0.3).to(BF)
    gn[C] = dict(x=gx, G=G, gamma=(1 + 0.2 * rnd(C)).to(BF), beta=(0.2 * rnd(C)).to(BF),
                 zy=rnd((Tg + 1) // 2, Hg // 2, Wg // 2, C).to(BF), zb=rnd((Tg + 1) // 2, Hg // 2, Wg // 2, C).to(BF),
                 part=rnd((Tg * Hg * Wg + 63) // 64 * (C // 4) * 2).abs())


def mx_bufs(K):
    return torch.empty(rows, K, device=dev, dtype=torch.uint8), torch.empty(K // 128, rows, 4, device=dev, dtype=torch.uint8)


def ln(xin, out_dtype, **kw):
    out = torch.empty(rows, D, device=dev, dtype=out_dtype)
    return lambda: ops.layernorm(xin, w, b, out, 1e-5, **kw)


def ln_mx(ww, bb, **kw):
    q, s = mx_bufs(D)
    return lambda: ops.layernorm_mxfp8(x, ww, bb, q, s, 1e-5, **kw)


def quant(xin):
    q, s = mx_bufs(xin.shape[1])
    return lambda: ops.quantize_mxfp8(xin, q, s)


def gemm_mx_out():
    a8, sa = ops.quantize_mxfp8(x); w8, sw = ops.quantize_mxfp8(w1)
    q, s = mx_bufs(4 * D)
    return lambda: (ops.gemm_mxfp8(a8, sa, w8, sw, out=q, out_scales=s, bias=b1, act="gelu_tanh"), s)


def split(**kw):
    def run():
        q, k, vt = (torch.zeros(B, H, Npad, 64, device=dev, dtype=BF) for _ in range(3))
        ops.qkv_split(qkv, q, k, vt.view(B, H, 64, Npad), B, N, H, Npad, **kw)
        return q, k, vt
    return run


def gn_stats(C):
    def run():
        st = torch.empty(Fg * gn[C]["G"] * 2, device=dev, dtype=torch.float64)
        ops.groupnorm_stats(gn[C]["x"], st, Fg, Tg * Hg * Wg, C, gn[C]["G"])
        return st
    return run


def gn_fold():
    st = torch.empty(32 * 2, device=dev, dtype=torch.float64)
    ops.groupnorm_stats_from_conv(gn[128]["part"], st, Tg * Hg * Wg, 128, 32)
    return st


def gn_apply(C, zq):
    d = gn[C]
    st = gn_stats(C)()
    def run():
        out = torch.zeros(Fg, Tg + 2, Hg + 2, Wg + 2, C, device=dev, dtype=BF)
        ops.groupnorm_apply(d["x"], out, st, d["gamma"], d["beta"], Fg, Tg, Hg, Wg, C, d["G"], zy=d["zy"] if zq else None,
                            zb=d["zb"] if zq else None, zshape=tuple(d["zy"].shape[:3]), tpad=2, hpad=1, wpad=1, swish=True)
        return out
    return run


CASES = [     # (name, thunk -> output tensors, timed)
    ("layernorm mod bf16->bf16", ln(x, BF, **mod), True), ("layernorm bf16->bf16", ln(x, BF), True),
    ("layernorm bf16->f32", ln(x, torch.float32), False), ("layernorm f32->bf16", ln(xf, BF), False),
    ("layernorm f32->f32", ln(xf, torch.float32), False), ("layernorm mod bf16->f32", ln(x, torch.float32, **mod), False),
    ("layernorm_mxfp8 mod", ln_mx(w, b, **mod), True), ("layernorm_mxfp8 plain", ln_mx(None, None), False),
    (f"quantize_mxfp8 K={D}", quant(x), True), (f"quantize_mxfp8 K={4 * D}", quant(x4), True),
    ("gemm_mxfp8 gelu -> mxfp8", None, True),
    ("qkv_split mode 0", split(ln=qk_ln), False), ("qkv_split mode 1", split(rope=rope), False), ("qkv_split mode 2", split(), False),
    ("groupnorm_stats C=128", gn_stats(128), False), ("groupnorm_stats C=24", gn_stats(24), False), ("groupnorm_stats_from_conv", gn_fold, False),
    ("groupnorm_apply rows zq", gn_apply(128, True), False), ("groupnorm_apply rows", gn_apply(128, False), False),
    ("groupnorm_apply flat zq", gn_apply(24, True), False), ("groupnorm_apply flat", gn_apply(24, False), False),
]


def digest(out):
    """Order-dependent 64-bit sums of the outputs' bytes, taken on the GPU."""
    h = 0
    for t in (out if isinstance(out, (tuple, list)) else (out,)):
        v = t.contiguous().view(torch.uint8).flatten()
        v = torch.nn.functional.pad(v, (0, -v.numel() % 8)).view(torch.int64)
        i = torch.arange(v.numel(), device=dev, dtype=torch.int64)
        h = (h * 1000003 + int(v.sum().item()) + int((v * (2 * i + 1)).sum().item())) & (2 ** 64 - 1)
    return f"{h:016x}"


def use(lib):
    _lib._lib = lib


print(f"rows {rows} (B {B} x N {N}, text {T}) D {D}; LD_LN_FAST={os.environ.get('LD_LN_FAST', '1')} LD_GN_ROWS={os.environ.get('LD_GN_ROWS', '1')}; "
      f"libraries: " + ", ".join(f"[{i}] {p}" for i, p in enumerate(paths)), flush=True)
for name, fn, timed in CASES:
    if only not in name:
        continue
    hashes, fns = [], []
    for lib in libs:
        use(lib)
        f = gemm_mx_out() if fn is None else fn
        hashes.append(digest(f())); fns.append(f)
    line = f"{name:28s} hash {hashes[0]} " + ("all equal" if len(set(hashes)) == 1 else "DIFFER: " + " ".join(hashes))
    if timed and not small:
        times = [[] for _ in libs]
        for rep in range(reps + 2):                               # the first two rounds warm up
            for i, lib in enumerate(libs):
                use(lib)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10): fns[i]()
                e1.record(); torch.cuda.synchronize()
                if rep >= 2: times[i].append(e0.elapsed_time(e1) / 10 * 1e3)
        line += "   us (median of %d x 10): " % reps + "  ".join(f"[{i}] {statistics.median(t):7.1f}" for i, t in enumerate(times))
    print(line, flush=True)
